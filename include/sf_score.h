/* sf_score.h — score poses against a map: frame-to-map agreement counts.
 *
 * A companion of sf.h, not part of its ABI: plain C declarations with the prefix sfs_, exported by libsf_hip.so (and its
 * precise and reference-order builds) only. The CPU oracle does not implement them and SF_ABI_VERSION does not count them;
 * sfs_version() versions this interface.
 *
 * The solver returns a pose per frame and nothing says whether that pose still explains the frame. These calls measure it
 * on the device, for many (map, view, frame) triples per call -- the same map and the same frame any number of times:
 *   - health: a stream's current frame against its own map at the pose the solver returned;
 *   - relocalisation search: one frame against one map at several hundred candidate poses;
 *   - change detection: where the frame lies in front of or behind the map (the class image).
 * A score call only READS its maps and streams: afterwards the map, sf_map_info, sf_map_get_index_map, the predictions,
 * the streams, the view scratch and sfv_last_large_sprites are what they were.
 *
 * THE MAP is drawn exactly as sf_view.h draws it (same culls, sprites, fragment test and 64-bit (depth, index) minimum)
 * into a key image of the score call's own scratch. A pixel is DRAWN when a fragment won it; zm is the camera z of the
 * winning fragment, gm the prediction's grey of the winner's colour bytes (the three bytes decoded from s[4]):
 *   f = (float)byte * (1.f / 255.f) per channel,  gm = (0.299f * fr + 0.587f * fg) + 0.114f * fb.
 * view.shade must be valid and is otherwise ignored.
 *
 * THE FRAME is a depth image zf, with use_grey an intensity image gf and with use_b a b image (the solver's per-pixel
 * static weight: the b image of the last solve masks what the solver itself called dynamic), all of the view's size,
 * column-major float32 like every image of sf.h: element (v, u) at v + u * rows.
 *
 * PER PIXEL, all arithmetic fp32 in the written order without contraction; a comparison with a NaN operand is false:
 *   fv     = zf > 0
 *   w      = use_b ? (b > b_min) : true
 *   F      = fv && w                 masked = fv && !w
 *   both   = F && drawn
 *   r      = zf - zm                 tol = tol_abs + tol_rel * zm
 *   inlier = both && fabsf(r) <= tol
 *   front  = both && r < -tol        (the frame is closer than the map)
 *   behind = both && r >  tol        (the frame sees through the map)
 *   q      = (int64)rintf(fminf(fabsf(r), max_residual) * 16384.f)
 * n_frame counts F, n_masked masked, n_map drawn, n_both, n_inlier, n_front, n_behind their predicates;
 *   sum_abs  = sum over both of q;   sum_sq = sum over both of q * q   (q <= 2^19 and <= 2^24 pixels: below 2^62);
 *   sum_grey = use_grey ? sum over inlier of (int64)rintf(fminf(fabsf(gf - gm), 1.f) * 65536.f) : 0.
 * fminf returns its other operand when one is a NaN, so a NaN gf adds 65536. The sums are integers, so they do not depend
 * on the order of summation: a score is a function of its inputs alone, for any batch composition and from run to run.
 * In metres: mean |r| = sum_abs / 16384 / n_both, rms = sqrt(sum_sq / n_both) / 16384; mean grey = sum_grey / 65536 / n_inlier.
 *
 * THE CLASS IMAGE is optional, uint8, column-major; every pixel gets exactly one code:
 *   0 neither frame nor map, 1 frame only, 2 map only (drawn, !fv), 3 inlier, 4 front, 5 behind, 6 masked (drawn or not).
 *
 * All functions return SF_OK or the SF_ERR_* codes of sf.h; sf_last_error() has the text.
 *
 * REFUSALS (SF_ERR_ARG unless said otherwise; nothing launched, nothing written): a null argument; n < 0 (n == 0 is
 * SF_OK); n > 65535; a map of another handle; a map whose handle was destroyed (SF_ERR_STATE); every refusal of
 * sfv_check_view; a stream index out of range (the code of sf_get_current); a view whose rows and cols are not the
 * handle's in the stream form; a NaN or inf in sfs_params; a negative tolerance; max_residual outside (0, 32]; a flag
 * other than 0 / 1; a flag set with its image missing; scratch that cannot be allocated (SF_ERR_NOMEM).
 */
#ifndef SF_SCORE_H_
#define SF_SCORE_H_

#include "sf_view.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sfs_params {
    float   tol_abs;       /* metres, >= 0 */
    float   tol_rel;       /* per metre of MAP depth, >= 0 */
    float   max_residual;  /* metres, 0 < . <= 32: |r| is clipped to it in the sums */
    float   b_min;         /* with use_b: a frame pixel counts when b > b_min */
    int32_t use_grey;      /* 0 / 1 */
    int32_t use_b;         /* 0 / 1 */
    int32_t reserved[2];   /* not read */
} sfs_params;              /* 32 bytes; sfs_params_bytes() reports it */

typedef struct sfs_score {
    int64_t n_frame, n_masked, n_map, n_both, n_inlier, n_front, n_behind;
    int64_t sum_abs, sum_sq, sum_grey;
    int64_t reserved[2];   /* written as 0 */
} sfs_score;               /* 96 bytes; sfs_score_bytes() reports it */

int sfs_version(void); /* 1 */
size_t sfs_params_bytes(void); /* sizeof(sfs_params) = 32 */
size_t sfs_score_bytes(void);  /* sizeof(sfs_score) = 96 */

/* tol_abs 0.02, tol_rel 0.01, max_residual 8, b_min 0.5, use_grey 1, use_b 1. These are parameter defaults, NOT acceptance
 * thresholds: nobody has tuned them on real data, and what inlier ratio means "lost" is the caller's to decide. */
int sfs_default_params(sfs_params *p);

/* Pure host, no handle, no GPU: SF_OK, or SF_ERR_ARG for null parameters or ones the refusal list names. */
int sfs_check_params(const sfs_params *p);

/* Entry q < n scores the current frame of streams[q] -- the level-0 depth and intensity sf_get_current returns and, with
 * use_b, the image sf_get_b_image returns, read on the device where they lie -- against maps[q] seen from views[q], whose
 * rows and cols must be the handle's. params and views hold n entries, scores is HOST memory for n records. class_out is
 * NULL or an array of n HOST pointers (rows * cols bytes each), any of which may be NULL. Ordered on the handle's HIP
 * stream; returns after the results are in host memory. */
int sfs_score_streams(sf_handle *h, int n, sf_map *const *maps, const sfv_view *views, const int32_t *streams, const sfs_params *params,
                      sfs_score *scores, uint8_t *const *class_out);

/* The same with frames in HOST memory: depth[q] (and grey[q], b[q]) of the size of views[q], 1 to 4096 rows and columns,
 * column-major float32 -- the output of sf_get_current goes straight in. grey and b are arrays of n pointers, or NULL; a
 * flag set in params[q] with its pointer missing is SF_ERR_ARG, a pointer whose flag is clear is not read. */
int sfs_score_images(sf_handle *h, int n, sf_map *const *maps, const sfv_view *views, const float *const *depth, const float *const *grey,
                     const float *const *b, const sfs_params *params, sfs_score *scores, uint8_t *const *class_out);

/* The same with DEVICE pointers in the (host) arrays depth, grey, b and class_out; scores is ONE device pointer to n
 * records. Asynchronous on the handle's stream; nothing is read back. */
int sfs_score_images_device(sf_handle *h, int n, sf_map *const *maps, const sfv_view *views, const void *const *depth, const void *const *grey,
                            const void *const *b, const sfs_params *params, void *scores, void *const *class_out);

#ifdef __cplusplus
}
#endif
#endif
