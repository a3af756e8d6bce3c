/* sf_tracks.h — region tracks: the moving regions of sf_regions.h followed from frame to frame, with a metric box.
 *
 * A companion of sf.h, not part of its ABI: plain C declarations with the prefix sft_, exported by libsf_hip.so (and its
 * precise and reference-order builds) only. The CPU oracle does not implement them and SF_ABI_VERSION does not count them;
 * sft_version() versions this interface.
 *
 * sf_regions.h numbers the regions of one frame by their smallest pixel index: region k of one frame has nothing to do with
 * region k of the next. A TRACKER gives regions an identity over time. Per followed camera (a SLOT) it keeps the previous
 * frame's regions on the device, warps them into the new frame with the two camera poses the caller hands in, counts for
 * every pair (previous track t, region k) the pixels that land in k, assigns greedily, and writes one integer record per
 * tracked region with its id, its age and its box and sums in WORLD coordinates. Everything behind a few fp32 operations in a
 * written order is an integer, so every id, count and sum is a function of the inputs alone.
 *
 * IMAGES are column-major float32 like every image of sf.h: element (v, u) at v + u * rows. All device arithmetic is fp32, one
 * rounding per operation in the written order, without contraction; a comparison with a NaN operand is false.
 *
 * CAMERA.  sft_camera: pose[16] is camera-to-world, column-major (entry (r, c) at r + 4 c); cx, cy, fx, fy in pixels.
 *
 * RELATIVE TRANSFORM.  D = sft_relative(prev.pose, cur.pose) takes previous-camera coordinates to current-camera coordinates.
 * With R0, t0 of the previous pose and R1, t1 of the current one, evaluated in fp64 and each entry rounded to float once:
 *   D[i + 4 j] = ((R1[0,i] R0[0,j] + R1[1,i] R0[1,j]) + R1[2,i] R0[2,j])      i, j < 3
 *   D[i + 12]  = ((R1[0,i] d0 + R1[1,i] d1) + R1[2,i] d2),  d = t0 - t1 in fp64
 *   D[3], D[7], D[11] = 0, D[15] = 1.
 * The transpose stands for the inverse: for a pose whose 3 x 3 is not orthonormal the result is what the formula gives. A
 * non-finite entry is refused. Equal poses give the exact identity.
 *
 * WARP of a previous pixel (v, u) with depth z, previous camera 0, current camera 1:
 *   P   = ((((float)u - cx0) * z) / fx0, (((float)v - cy0) * z) / fy0, z)
 *   h_i = ((D[i] P.x + D[i+4] P.y) + D[i+8] P.z) + D[i+12]                     i < 3
 *   dropped unless h.z > 0
 *   uf  = ((fx1 * h.x) / h.z) + cx1,   vf = ((fy1 * h.y) / h.z) + cy1
 *   ui  = floorf(uf + 0.5f),           vi = floorf(vf + 0.5f)
 *   kept when ui >= 0 && ui < cols && vi >= 0 && vi < rows, tested as floats before any conversion.
 *
 * A TRACKER is created from a handle for one rows x cols, with n_slots slots (1..65535) and max_tracks M (1..256). It is
 * ordered on the handle's stream and released by sft_tracker_destroy, or by the handle's sf_destroy, which leaves a shell on
 * which every call but sft_tracker_destroy returns SF_ERR_STATE. Per slot, in device memory: the previous frame's clipped label
 * image (int32: k in 1..K_prev, else 0), its depth and its camera; per row 1..K_prev the track id, the birth frame and the
 * pixel count; `frames`, and `next_id`, which starts at 1. Ids belong to one slot and are never reused.
 *
 * UPDATE of slot s with a frame (depth Z, static weight B, camera C1, region parameters rp, track parameters tp):
 *  1 REGIONS.  The regions of the frame are exactly those of sf_regions.h under rp: label image L, R regions, records.
 *    K = min(R, M). Regions above K are untracked: their id is 0 and n_untracked counts them.
 *  2 OVERLAP.  If the slot has a previous frame: every previous pixel p with clipped label t in 1..K_prev that the warp keeps
 *    at (vi, ui) counts in n_warped. With k = L(vi, ui) in 1..K it counts in O[t][k] when tp.use_depth_gate == 0 or
 *      fabsf(h.z - Z(vi,ui)) <= tp.dz_abs + tp.dz_rel * fminf(h.z, Z(vi,ui)).
 *    Several sources may land on one pixel and each one counts.
 *  3 ASSIGNMENT.  Greedy and fully ordered. (t, k) is a candidate when, in int64, O[t][k] >= tp.min_overlap and
 *      1024 * O[t][k] >= tp.min_share * min(n_prev[t], n_cur[k]).
 *    Candidates are walked by O descending, then t ascending, then k ascending; a pair is taken when neither side is taken
 *    yet. A matched region keeps t's id and birth frame. Unmatched regions k <= K are born in ascending k with id = next_id++
 *    and birth frame = the slot's `frames` before this update. Unmatched previous tracks end.
 *  4 TRACK RECORD.  Each of the K rows gets an sft_track: id, region (k), prev_region (t or 0), birth_frame, age (frames before
 *    this update - birth_frame), overlap (O[t][k] or 0); the 2-D fields of the region record; and the world-frame box and sums.
 *    For every pixel (v, u) of the region with depth z:
 *      P1  = ((((float)u - cx1) * z) / fx1, (((float)v - cy1) * z) / fy1, z)
 *      W_i = ((pose1[i] P1.x + pose1[i+4] P1.y) + pose1[i+8] P1.z) + pose1[i+12]
 *      q_i = (int32)rintf(fminf(fmaxf(W_i, -2048.f), 2048.f) * 1024.f)          (fmaxf of a NaN gives the other operand)
 *    and the record holds qmin[3], qmax[3] and int64 sum_q[3]. The centroid is sum_q / n / 1024 metres; the velocity between two
 *    updates is the caller's difference of centroids. Records K .. M - 1 of an entry are written as zeros.
 *  5 SUMMARY.  sft_summary: n_regions R, n_tracked K, n_matched, n_born, n_ended, n_untracked R - K, n_warped, next_id (after).
 *  6 ID IMAGE (int32, column-major, optional): the track id per pixel, 0 elsewhere (untracked regions included).
 *  7 COMMIT.  The slot's previous frame becomes this one, and frames += 1.
 * The first update of a slot, and the first after sft_reset_slots, skips steps 2 and 3: everything is a birth, n_warped and
 * n_ended are 0.
 *
 * All functions return SF_OK or the SF_ERR_* codes of sf.h; sf_last_error() has the text.
 *
 * REFUSALS (SF_ERR_ARG unless said otherwise; nothing launched, no state changed, no output written): a null argument; n < 0
 * or n > 65535 (n == 0 is SF_OK); a slot out of range; the same slot twice in one call; a size that is not the tracker's; in
 * the stream form a tracker whose size is not the handle's, or a stream index out of range (the code of sf_get_current); a
 * non-finite camera entry, or fx or fy equal to 0; every refusal of sfr_params (use_b without a b image among them);
 * min_overlap < 1; min_share outside 0..1024; a negative or non-finite dz_abs or dz_rel; use_depth_gate other than 0 / 1; a
 * tracker of a destroyed handle (SF_ERR_STATE); scratch that cannot be grown (the allocation's own code).
 *
 * NOT HERE: re-identifying a track after frames in which it was not seen (an unmatched track ends), motion models and
 * prediction, the rigid motion of a region, tracks across slots, checkpointing a tracker, and regions of the map.
 */
#ifndef SF_TRACKS_H_
#define SF_TRACKS_H_

#include "sf_regions.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sft_tracker sft_tracker;

typedef struct sft_camera {
    float pose[16];        /* camera-to-world, column-major */
    float cx, cy, fx, fy;  /* pixels; fx, fy != 0 */
} sft_camera;              /* 80 bytes; sft_camera_bytes() reports it */

typedef struct sft_params {
    int32_t min_overlap;     /* >= 1 */
    int32_t min_share;       /* 0..1024: 1024ths of the smaller of the two pixel counts */
    int32_t use_depth_gate;  /* 0 / 1 */
    float   dz_abs;          /* metres, >= 0 */
    float   dz_rel;          /* per metre of the nearer depth, >= 0 */
    int32_t reserved[3];     /* not read */
} sft_params;                /* 32 bytes; sft_params_bytes() reports it */

typedef struct sft_track {
    int32_t id, region, prev_region, birth_frame, age, overlap;
    int32_t n, first, v_min, v_max, u_min, u_max, z_min, z_max; /* as in sfr_region */
    int32_t qmin[3], qmax[3];                                   /* world box, 1024ths of a metre */
    int64_t sum_v, sum_u, sum_z, sum_b;                         /* as in sfr_region */
    int64_t sum_q[3];                                           /* world sums, 1024ths of a metre */
} sft_track;                 /* 136 bytes; sft_track_bytes() reports it */

typedef struct sft_summary {
    int32_t n_regions, n_tracked, n_matched, n_born, n_ended, n_untracked, n_warped, next_id;
} sft_summary;               /* 32 bytes; sft_summary_bytes() reports it */

typedef struct sft_info {
    int32_t rows, cols, n_slots, max_tracks;
    int32_t reserved[4];     /* written as 0 */
} sft_info;                  /* 32 bytes; sft_info_bytes() reports it */

typedef struct sft_slot {
    int32_t frames;          /* updates since creation or the last reset with restart_ids */
    int32_t next_id;         /* the id the next birth gets */
    int32_t n_tracks;        /* K of the last update; 0 when the slot holds no previous frame */
    int32_t reserved;        /* written as 0 */
} sft_slot;                  /* 16 bytes; sft_slot_bytes() reports it */

int sft_version(void); /* 1 */
size_t sft_camera_bytes(void);  /* 80 */
size_t sft_params_bytes(void);  /* 32 */
size_t sft_track_bytes(void);   /* 136 */
size_t sft_summary_bytes(void); /* 32 */
size_t sft_info_bytes(void);    /* 32 */
size_t sft_slot_bytes(void);    /* 16 */

/* min_overlap 1, min_share 256, use_depth_gate 1, dz_abs 0.10, dz_rel 0.05. These are parameter defaults, NOT tuned values:
 * nobody has tuned them on real data. */
int sft_default_params(sft_params *p);

/* Pure host, no handle, no GPU: SF_OK, or SF_ERR_ARG for null parameters or ones the refusal list names. */
int sft_check_params(const sft_params *p);

/* Pure host: the relative transform of two camera-to-world poses, as defined above. */
int sft_relative(const float prev_pose[16], const float cur_pose[16], float d_out[16]);

/* Pure host: step 3 on a caller's table. overlap is k_prev x k, row t - 1 at (t - 1) * k; n_prev holds k_prev counts, n_cur
 * k; k_prev and k lie in 0..256. prev_of_cur_out (k entries) gets the t of the track region k took, or 0; cur_of_prev_out
 * (k_prev entries, may be NULL) the k a track went to, or 0; *n_matched_out (may be NULL) the number of pairs taken. The
 * device runs the same program text. */
int sft_assign(int k_prev, int k, const int32_t *overlap, const int32_t *n_prev, const int32_t *n_cur, int min_overlap, int min_share,
               int32_t *prev_of_cur_out, int32_t *cur_of_prev_out, int32_t *n_matched_out);

/* rows and cols in 1..4096 with rows * cols <= 2^24 (the images of sf_regions.h), n_slots in 1..65535, max_tracks in 1..256.
 * SF_ERR_NOMEM when the slots do not fit the device. */
int sft_tracker_create(sf_handle *h, int rows, int cols, int n_slots, int max_tracks, sft_tracker **out);
void sft_tracker_destroy(sft_tracker *t);
int sft_tracker_info(const sft_tracker *t, sft_info *info_out);

/* Host side: waits for the handle's stream, then reads the slot's counters from the device. */
int sft_slot_info(sft_tracker *t, int slot, sft_slot *slot_out);

/* The n slots forget their previous frame: their next update is a first update. With restart_ids != 0 their next_id goes
 * back to 1 and their frames to 0; otherwise both go on counting. Ordered on the handle's stream. */
int sft_reset_slots(sft_tracker *t, int n, const int32_t *slots, int restart_ids);

/* Entry q < n updates slot slots[q] with the current frame of streams[q]: the level-0 depth sf_get_current returns and the
 * image sf_get_b_image returns, read on the device where they lie. cameras, rparams and tparams hold n entries;
 * summaries_out is HOST memory for n records, tracks_out HOST memory for n * max_tracks records (entry q at q * max_tracks).
 * ids_out is NULL or an array of n HOST pointers (rows * cols int32 each), any of which may be NULL. Returns after the
 * results are in host memory. */
int sft_update_streams(sft_tracker *t, int n, const int32_t *slots, const int32_t *streams, const sft_camera *cameras, const sfr_params *rparams,
                       const sft_params *tparams, sft_summary *summaries_out, sft_track *tracks_out, int32_t *const *ids_out);

/* The same with frames in HOST memory: depth[q] (and b[q]) of rows x cols, the tracker's size. b is an array of n pointers,
 * or NULL when no entry sets use_b; a pointer whose entry's use_b is clear is not read. */
int sft_update_images(sft_tracker *t, int rows, int cols, int n, const int32_t *slots, const float *const *depth, const float *const *b,
                      const sft_camera *cameras, const sfr_params *rparams, const sft_params *tparams, sft_summary *summaries_out, sft_track *tracks_out,
                      int32_t *const *ids_out);

/* The same with DEVICE pointers in the (host) arrays depth, b and ids_out; summaries_out and tracks_out are ONE device
 * pointer each, to n and to n * max_tracks records, 8-byte aligned. Asynchronous on the handle's stream; nothing is read
 * back, which is why next_id lives on the device. */
int sft_update_images_device(sft_tracker *t, int rows, int cols, int n, const int32_t *slots, const void *const *depth, const void *const *b,
                             const sft_camera *cameras, const sfr_params *rparams, const sft_params *tparams, void *summaries_out, void *tracks_out,
                             void *const *ids_out);

#ifdef __cplusplus
}
#endif
#endif
