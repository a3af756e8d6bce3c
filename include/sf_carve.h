/* sf_carve.h — carve surfel maps by what later frames saw through them.
 *
 * A companion of sf.h, not part of its ABI: plain C declarations with the prefix sfe_, exported by libsf_hip.so (and its
 * precise and reference-order builds) only. The CPU oracle does not implement them and SF_ABI_VERSION does not count them;
 * sfe_version() versions this interface.
 *
 * A map loses surfels by age, distance or confidence (sfw_cull_maps), by voxel density (the thinning of the join), by going
 * stale while unstable (the clean stage of a fuse) and by the window test inside a fuse. Nothing removes a surfel because a
 * frame looked straight through it: a thing that stood still until it was stable and was then carried away leaves a ghost.
 * sfs_score_* of sf_score.h already SEES that (n_behind, class 5), per pixel and for the front-most surfel only. This
 * interface is its companion: the score says THAT a map is wrong, a carve says WHICH surfels, and takes them out.
 *
 * A CALL takes n_maps DISTINCT maps, each with its own sfe_params and sfe_counts, and n ENTRIES. Entry q is a map index
 * map_of[q] in 0 .. n_maps - 1, a view views[q] (sfv_view of sf_view.h: the pose and intrinsics the frame was taken with, and
 * the culls of a render) and a depth frame zf of the view's size, column-major float32 like every image of sf.h: element
 * (v, u) at v + u * rows. Any number of entries may name the same map -- several frames vote on one map --, and a map may
 * have no entries. The frame comes in one of two forms, as in sf_score.h: the level-0 depth of a stream of the handle, read
 * on the device where it lies (sfe_carve_streams), or a host image (sfe_carve_images).
 *
 * DEFINITIONS. s[0..11] is a surfel in the layout of sf.h. All arithmetic is fp32, one rounding per operation in the written
 * order, without contraction; a comparison with a NaN operand is false. pdot(a, b) = a.x*b.x + a.y*b.y + a.z*b.z.
 *
 * OBSERVE, one surfel s against one entry of its map; tick is the map's:
 *   T = inverse(view.pose)                               the routine the views use
 *   h.k = ((T[k]*s0 + T[4+k]*s1) + T[8+k]*s2) + T[12+k]  the camera position the views compute
 *   m.k =  (T[k]*s8 + T[4+k]*s9) + T[8+k]*s10            NOT normalised: there is no square root in this rule
 *   UNSEEN when the view culls s exactly as sf_view.h does:
 *          h.z > max_depth, h.z < 0.4f, s[3] < min_confidence, or (max_age >= 0 and not (float)tick - s[7] <= (float)max_age)
 *   d = pdot(m, h);  mm = pdot(m, m);  hh = pdot(h, h)
 *   UNSEEN unless  d < 0  &&  d*d >= (min_cos*min_cos) * (mm*hh)      it faces the camera and is not seen at a grazing angle
 *   qx = ((fx*h.x)/h.z + cx) + 0.5f;   qy = ((fy*h.y)/h.z + cy) + 0.5f
 *          frames have their pixel centres at integers (pixel (v, u) is the ray ((u - cx)/fx, (v - cy)/fy, 1))
 *   UNSEEN unless  qx >= 0 && qx < (float)cols && qy >= 0 && qy < (float)rows
 *   i = (int)floorf(qx);  j = (int)floorf(qy);  w = window
 *   for ii = i-w .. i+w (outer), jj = j-w .. j+w, inside the image:
 *       z  = zf[jj + ii*rows]                        valid  = z > 0 && z <= z_max
 *       lx = ((float)ii - cx)/fx;  ly = ((float)jj - cy)/fy
 *       den = (lx*m.x + ly*m.y) + m.z;  zp = d/den   valid &= zp >= 0.4f && zp <= max_depth
 *       tol = tol_abs + tol_rel*zp;     r = z - zp
 *       through += valid && r > tol;  near += valid && fabsf(r) <= tol;  front += valid && r < -tol
 *   class:  near > 0 -> SUPPORTED (2);  else through >= min_pixels -> THROUGH (1);
 *           else front > 0 -> OCCLUDED (3);  else UNSEEN (0)
 * zp is the camera z at which THAT PIXEL'S ray meets the surfel's plane -- the fragment depth of the views --, not h.z: on a
 * floor seen at a grazing angle the depth of the centre is off by more than any sensible tolerance one pixel further on.
 * view.shade must be valid and is otherwise ignored.
 *
 * DECIDE, per surfel over the entries of its map: v_through = the number of entries with class THROUGH, v_support = the number
 * with class SUPPORTED (both at most 65535, because a call has at most 65535 entries); OCCLUDED and UNSEEN vote for nothing.
 *   carved = v_through >= min_votes && v_support <= max_support
 * The votes are integers: no result depends on an order of arrival, on the order of the entries or on what else is in the call.
 *
 * EFFECT. The surfels that are not carved stay, bit for bit and in their old order: the stable partition of
 * sf_map_window.h under the predicate. A map with n_carved == 0, or under dry_run, or with no entries, is
 * NOT TOUCHED AT ALL: its buffer is not swapped and sf_map_get_index_map keeps working. Otherwise the rule
 * AFTER A CALL THAT CHANGES A MAP of sf_map_window.h holds: the count is n_out, tick, pose and statistics stay, sf_map_get_index_map answers SF_ERR_STATE
 * until the next fuse, and prediction, fusion and download work on the carved map. Everything else is only read: the
 * streams, the other maps, the view scratch and sfv_last_large_sprites, and the scratch of every other interface. Votes are
 * not kept from call to call.
 *
 * COUNTS, one sfe_counts per map, each "in at least one entry": n_in (the old count), n_judged (any class other than UNSEEN),
 * n_through, n_supported, n_occluded, n_carved, n_out = n_in - n_carved, reserved = 0.
 * VOTES, optional: votes_out is NULL, or n_maps host pointers each of which may be NULL; a pointer that is not has room for the
 * map's OLD count of uint32_t and receives v_through | v_support << 16 per surfel, in the OLD order.
 *
 * Both carve calls are ordered on the handle's HIP stream and return after the counts are in host memory; there is no
 * device-output form, because the host needs the counts to set the maps' counts.
 *
 * All functions return SF_OK or the SF_ERR_* codes of sf.h; sf_last_error() has the text.
 *
 * REFUSALS (SF_ERR_ARG unless said otherwise; nothing is launched, nothing is changed, no output is written): a null argument
 * (votes_out may be null; with n == 0, map_of, views and the frames may be null too); n or n_maps below 0 or above 65535
 * (0 is SF_OK); a map_of[q] out of range; the same map twice; a map of another handle than the carver's; a shell carver, or a
 * map whose handle is gone (SF_ERR_STATE); every refusal of sfv_check_view; a stream index out of range, or a view that is
 * not the handle's size in the stream form; a host image size outside rows, cols in 1..4096 with rows * cols <= 2^24; a null
 * depth image; params with a NaN or inf, a negative tolerance, z_max outside (0, 32], min_cos outside [0, 1], window outside
 * 0..3, min_pixels outside 1..(2 window + 1)^2, min_votes outside 1..65535, max_support outside 0..65535, dry_run not 0 or 1;
 * scratch that cannot be grown (the allocation's own code).
 *
 * UNMEASURED: nobody has tuned the defaults, and nobody has measured what a carve does to maps of real
 * sequences (sensor noise at depth edges, poses that are slightly off). min_votes = 2 asks for two frames before anything
 * goes; max_support = 0 lets one frame that still sees the surface keep it.
 * NORMALS. "Faces the camera" is d < 0: the normal points from the surface towards the camera. sf_map_fuse_frame stores the
 * normal of its data association the other way round (away from the camera that saw the surface, d > 0), which the drawing
 * of sf_view.h does not mind and this rule does: every surfel of a map as fused is UNSEEN, and a carve takes nothing from it.
 * A caller carves maps whose normals face the frames' cameras (uploaded or appended surfels, or a fused map with its normals
 * negated); which sign the rule should accept for fused maps is open.
 *
 * OUT OF SCOPE: b images and photometric evidence; lowering confidence instead of removing surfels;
 * votes kept from call to call; paging the carved surfels out; a device-pointer form; writing anything into a stream.
 */
#ifndef SF_CARVE_H_
#define SF_CARVE_H_

#include "sf.h"
#include "sf_view.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the classes sfe_observe returns */
#define SFE_CLASS_UNSEEN 0
#define SFE_CLASS_THROUGH 1
#define SFE_CLASS_SUPPORTED 2
#define SFE_CLASS_OCCLUDED 3
#define SFE_MAX_WINDOW 3

typedef struct sfe_carver sfe_carver;

typedef struct sfe_params {
    float   tol_abs;      /* metres, >= 0                                                                    */
    float   tol_rel;      /* per metre of zp, >= 0                                                           */
    float   z_max;        /* metres, 0 < . <= 32: a frame depth beyond it is no evidence                     */
    float   min_cos;      /* 0 .. 1: the cosine between normal and view ray below which a surfel is UNSEEN   */
    int32_t window;       /* 0 .. 3: the window is (2 window + 1)^2 pixels                                   */
    int32_t min_pixels;   /* 1 .. (2 window + 1)^2: pixels that must see through for the class THROUGH       */
    int32_t min_votes;    /* 1 .. 65535: entries that must see through for a surfel to be carved             */
    int32_t max_support;  /* 0 .. 65535: entries that may still support a carved surfel                      */
    int32_t dry_run;      /* 0 / 1: count and vote, change nothing                                           */
    int32_t reserved[3];  /* not read                                                                        */
} sfe_params;             /* 48 bytes; sfe_params_bytes() reports it */

typedef struct sfe_counts {
    int32_t n_in;         /* the map's count before the call           */
    int32_t n_judged;     /* any class other than UNSEEN, in >= 1 entry */
    int32_t n_through;    /* THROUGH in >= 1 entry                      */
    int32_t n_supported;  /* SUPPORTED in >= 1 entry                    */
    int32_t n_occluded;   /* OCCLUDED in >= 1 entry                     */
    int32_t n_carved;
    int32_t n_out;        /* n_in - n_carved                            */
    int32_t reserved;     /* 0                                          */
} sfe_counts;             /* 32 bytes; sfe_counts_bytes() reports it */

int sfe_version(void); /* 1 */
size_t sfe_params_bytes(void); /* 48 */
size_t sfe_counts_bytes(void); /* 32 */

/* tol_abs 0.02, tol_rel 0.01, z_max 8, min_cos 0.2, window 1, min_pixels 5, min_votes 2, max_support 0, dry_run 0. These are
 * parameter defaults, NOT tuned values. */
int sfe_default_params(sfe_params *p);

/* Pure host, no handle, no GPU: SF_OK, or SF_ERR_ARG for null parameters or ones the refusal list names. */
int sfe_check_params(const sfe_params *p);

/* Pure host; the device compiles the same text. OBSERVE for one surfel s of a map at `tick` against `view` and the depth
 * image `depth` of the view's size: found[0..2] = through, near, front. Returns the class (SFE_CLASS_*), or SF_ERR_ARG
 * (negative) for a null argument, a view sfv_check_view refuses, an image size the refusal list names, or bad params. */
int sfe_observe(const float s[12], int tick, const sfv_view *view, const float *depth, const sfe_params *params, int32_t found[3]);

/* Pure host; the device compiles the same text. DECIDE: 1 carved, 0 not; SF_ERR_ARG (negative) for votes outside 0..65535 or
 * bad params. */
int sfe_decide(int v_through, int v_support, const sfe_params *params);

/* A carver on h. It owns the device memory its calls use; sf_destroy of h releases the memory and leaves a shell that every
 * call answers with SF_ERR_STATE and sfe_carver_destroy frees. */
int sfe_carver_create(sf_handle *h, sfe_carver **out);
void sfe_carver_destroy(sfe_carver *carver);

/* Entry q < n is the current frame of streams[q] -- the level-0 depth sf_get_current returns, read on the device where it
 * lies -- seen from views[q], whose rows and cols must be the handle's, voting on maps[map_of[q]]. params and counts_out hold
 * n_maps records; votes_out is NULL or n_maps HOST pointers. */
int sfe_carve_streams(sfe_carver *carver, int n_maps, sf_map *const *maps, const sfe_params *params, int n, const int32_t *map_of, const sfv_view *views,
                      const int32_t *streams, sfe_counts *counts_out, uint32_t *const *votes_out);

/* The same with frames in HOST memory: depth[q] of the size of views[q], column-major float32 -- the output of
 * sf_get_current goes straight in. */
int sfe_carve_images(sfe_carver *carver, int n_maps, sf_map *const *maps, const sfe_params *params, int n, const int32_t *map_of, const sfv_view *views,
                     const float *const *depth, sfe_counts *counts_out, uint32_t *const *votes_out);

#ifdef __cplusplus
}
#endif
#endif
