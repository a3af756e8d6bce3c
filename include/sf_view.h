/* sf_view.h — render surfel maps from any view: depth, colour and index images.
 *
 * A companion of sf.h, not part of its ABI: plain C declarations with the prefix sfv_, exported by libsf_hip.so (and its
 * precise and reference-order builds) only. The CPU oracle does not implement them and SF_ABI_VERSION does not count them;
 * sfv_version() versions this interface.
 *
 * sf_map_predict* draws a map from the map's own pose, at the handle's resolution and intrinsics, mixes the previous frame
 * in and hands depth and grey to the solver. These calls are the compute half of "show me the map from here": any pose, any
 * pinhole intrinsics, any size up to 4096 x 4096, no fill-in, and the images come back to the caller -- thumbnails of many
 * maps, a look at a map after sfw_cull_maps / sfw_page_out or after a resume, depth or colour from a virtual camera. A render
 * only READS its maps: the same map may appear any number of times in one call, and afterwards the map, sf_map_info,
 * sf_map_get_index_map, sf_get_prediction and sf_get_prediction_dense_stream are what they were.
 *
 * GEOMETRY. One target of IndexMap::combinedPredict, as the prediction draws it: s[0..11] is a surfel in the layout of sf.h.
 * With T = inverse(pose) (the routine the prediction uses), h = T * s[0..2] and the camera-frame normal n,
 *   - the surfel is culled when h.z > max_depth, h.z < 0.4f, s[3] < min_confidence, or (max_age >= 0 and not
 *     (float)tick - s[7] <= (float)max_age); a comparison with a NaN operand is false;
 *   - a surfel whose centre projects outside the image is not drawn (splat.vert); the sprite is the square around the
 *     centre whose side is the longer extent of the four projected corners; while all four corners have z > 0 only the
 *     pixels of their bounding rectangle (widened by one pixel) are visited, which loses no fragment (the disc lies inside
 *     the diamond of the corners); a surfel with a corner at z <= 0 keeps the whole square;
 *   - per fragment: the view ray of the pixel centre meets the surfel's plane; the fragment is kept inside the disc of
 *     radius s[11], with depth = z / (2 max_depth) + 0.5 kept when 0 <= depth < 1;
 *   - the smallest (depth, surfel index) wins a pixel, so the earlier surfel wins an exact tie.
 * All arithmetic is fp32 in the written order, without contraction: the images are a function of the inputs alone, bit for
 * bit the same from run to run and for any batch composition.
 *
 * OUTPUTS, all row-major rows x cols: depth float32 (metres, camera z of the winning fragment, 0 where nothing was drawn;
 * no extract_max_depth clip), rgb uint8 x 3 (0,0,0 where nothing was drawn), index int32 (position of the winning surfel
 * in the map's buffer, -1 where nothing was drawn: surfels[index] gives a caller every other attribute).
 *
 * All functions return SF_OK or the SF_ERR_* codes of sf.h; sf_last_error() has the text.
 *
 * REFUSALS (SF_ERR_ARG unless said otherwise; nothing launched, nothing written): a null argument; n < 0 (n == 0 is
 * SF_OK); n > 65535; a map of another handle; a NaN or inf anywhere in a view; rows or cols outside 1..4096; fx or fy equal
 * to 0; max_depth <= 0.4; an unknown shade; a map whose handle was destroyed (SF_ERR_STATE); scratch that cannot be
 * allocated (SF_ERR_NOMEM).
 */
#ifndef SF_VIEW_H_
#define SF_VIEW_H_

#include "sf.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SFV_SHADE_COLOUR = 0, SFV_SHADE_NORMAL = 1 };
/* SFV_SHADE_COLOUR: the three bytes decoded from s[4]. SFV_SHADE_NORMAL: with n the normalised camera-frame normal of the
 * winner, channel k = (uint8_t)(int)rintf(fminf(fmaxf(0.5f * n[k] + 0.5f, 0.f), 1.f) * 255.f). */

typedef struct sfv_view {
    float   pose[16];        /* camera-to-world, column-major, like currPose */
    float   cx, cy, fx, fy;  /* pinhole intrinsics of THIS view, pixels */
    int32_t rows, cols;      /* 1..4096 each, independent of the handle's resolution */
    float   min_confidence;  /* a surfel is drawn when !(s[3] < min_confidence); 0 draws unstable ones too */
    float   max_depth;       /* > 0.4: camera z beyond it is culled; also scales the depth key, as maxDepthProcessed does */
    int32_t max_age;         /* >= 0 enables (float)tick - s[7] <= (float)max_age with the map's tick (test B of sfw_filter); < 0: off */
    int32_t shade;           /* SFV_SHADE_* */
    int32_t reserved[2];     /* pads the struct to 112 bytes; not read */
} sfv_view;                  /* 112 bytes; sfv_view_bytes() reports it */

int sfv_version(void); /* 1 */
size_t sfv_view_bytes(void); /* sizeof(sfv_view) = 112 */

/* Pure host, no handle, no GPU: SF_OK, or SF_ERR_ARG for a null view or one the refusal list names. */
int sfv_check_view(const sfv_view *v);

/* The handle's resolution, the intrinsics of sf_default_model_params, max_depth 20, min_confidence 0.25 (the drivers'
 * confidenceThreshold), max_age -1, colour shading; the pose of `m`, or identity when m is NULL. */
int sfv_default_view(const sf_handle *h, sf_map *m, sfv_view *v);

/* views[q] of maps[q] for q < n, in one set of launches. depth_out, rgb_out and index_out are arrays of n HOST pointers;
 * any of the three arrays may be NULL, and so may any entry: that image is not produced. The views of a call may differ
 * in size; the same map may appear any number of times. Ordered on the handle's HIP stream; returns after the images are
 * in host memory. */
int sfv_render_maps(sf_handle *h, int n, sf_map *const *maps, const sfv_view *views, float *const *depth_out, uint8_t *const *rgb_out,
                    int32_t *const *index_out);

/* The same with DEVICE pointers in the three (host) arrays. Asynchronous on the handle's stream; nothing is read back. */
int sfv_render_maps_device(sf_handle *h, int n, sf_map *const *maps, const sfv_view *views, void *const *depth_out, void *const *rgb_out,
                           void *const *index_out);

/* One view of `count` surfels in host memory, without a map: what sfw_extract / sfw_page_out returned, or what a checkpoint
 * holds. `tick` stands in for the map's tick in the age test. Uploaded to the handle's view scratch, then drawn by the
 * same kernels. depth, rgb and index are host pointers; each may be NULL. */
int sfv_render_surfels(sf_handle *h, const float *surfels, int count, int tick, const sfv_view *view, float *depth, uint8_t *rgb, int32_t *index);

/* How many surfels of each view of the handle's LAST render call were drawn as large sprites (a clipped sprite of more
 * than 32 x 32 = 1024 pixels is drawn by a whole wave instead of one lane; the images do not depend on it). counts holds
 * n entries, n = the n of that call (1 after sfv_render_surfels); another n, or no render yet: SF_ERR_STATE. */
int sfv_last_large_sprites(sf_handle *h, int n, int32_t *counts);

#ifdef __cplusplus
}
#endif
#endif
