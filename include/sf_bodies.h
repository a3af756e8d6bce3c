/* sf_bodies.h — region motion: the rigid motion of every moving region between two frames, by point-to-plane steps.
 *
 * A companion of sf.h, not part of its ABI: plain C declarations with the prefix sfb_ ("bodies"), exported by libsf_hip.so
 * (and its precise and reference-order builds) only. The CPU oracle does not implement them and SF_ABI_VERSION does not count
 * them; sfb_version() versions this interface.
 *
 * sf_regions.h says what moved and sf_tracks.h whether it is the same thing as a frame ago. The difference of two track
 * centroids is the centroid of a visible cap and says nothing about rotation. These calls align, per region, the region's
 * pixels of the earlier frame with the surface of the later frame: many regions per frame pair, many frame pairs per call,
 * on the device, without a host synchronisation between iterations. A call only READS its inputs: afterwards the streams,
 * maps, predictions, trackers and the scratch results of every other companion are what they were.
 *
 * IMAGES are column-major like every image of sf.h: element (v, u) at v + u * rows; depths float32, labels int32. All pixel
 * arithmetic is fp32, one rounding per operation in the written order, without contraction; a comparison with a NaN
 * operand is false.
 *   pdot(a, b)   = (a.x * b.x + a.y * b.y) + a.z * b.z
 *   pcross(a, b) = (a.y * b.z - b.y * a.z,  a.z * b.x - b.z * a.x,  a.x * b.y - b.x * a.y)
 *
 * AN ENTRY is a pair of frames of one size: frame 0 (earlier) with depth Z0, label image L0 and camera C0; frame 1 with depth
 * Z1, optionally a label image L1, and camera C1. Cameras are sfb_camera, the camera of sf_tracks.h field for field.
 * K = n_regions[q] (0..M) is the number of regions of the entry and M = max_regions (1..256) is the same for every entry of the
 * call. A pixel whose L0 lies outside 1..K (0, negative, larger) belongs to no region. pairs (optional) holds n * M int32:
 * pairs[q * M + t - 1] names the label of L1 that region t must land on, 0 for any pixel of frame 1; with tracks it is the
 * `region` of the track record whose prev_region is t. Entries t > K of a row of pairs are checked like the others and
 * otherwise not used.
 *
 * BACK-PROJECTION, the fusion convention of sf_tracks.h, with the intrinsics of the frame's own camera:
 *   P(v, u, z) = ((((float)u - cx) * z) / fx,  (((float)v - cy) * z) / fy,  z)
 *
 * TARGET MODEL of frame 1, computed once per entry.  valid1 = Z1 > 0 && Z1 <= z_max. A pixel (v, u) has a normal when
 * 1 <= v <= rows - 2 and 1 <= u <= cols - 2, it and its four neighbours are valid1, and fabsf(Zn - Z) <= normal_dz for each
 * of the four neighbour depths Zn; and then, with P1 = P under C1,
 *   a = P1(v, u + 1) - P1(v, u - 1)      b = P1(v + 1, u) - P1(v - 1, u)       (component by component)
 *   c = pcross(a, b)                     cc = pdot(c, c)
 *   the pixel has a normal iff cc > 0 && cc < INFINITY;   s = sqrtf(cc),   n = (c.x / s, c.y / s, c.z / s).
 * Frames with fewer than 3 rows or columns have no normals. The sign of n is left as computed: every sum below is even in n.
 *
 * THE ESTIMATE of a region is a 3 x 4 matrix D, row-major D[k][c] = D[4 * k + c] as in sf_align.h, that takes frame-0 camera
 * coordinates of the body to frame-1 camera coordinates. It is carried in fp64 and used by the pixel pass rounded to float.
 * Every region of an entry starts at D0 = the RELATIVE TRANSFORM of sf_tracks.h of (C0.pose, C1.pose),
 * D0[k][c] = (double)rel[k + 4 * c]: the hypothesis "it did not move in the room".
 *
 * LINEARISATION of region t at D, over the pixels (v, u) with L0 == t, z = Z0(v, u):
 *  1 ok  = z > 0 && z <= z_max
 *  2 P   = P(v, u, z) under C0;   Q.k = ((D[k][0] * P.x + D[k][1] * P.y) + D[k][2] * P.z) + D[k][3];   ok &= Q.z > 0
 *  3 the WARP of sf_tracks.h:  uf = ((fx1 * Q.x) / Q.z) + cx1,  vf = ((fy1 * Q.y) / Q.z) + cy1,  ui = floorf(uf + 0.5f),
 *    vi = floorf(vf + 0.5f);  ok &= ui >= 0 && ui < cols && vi >= 0 && vi < rows, tested as floats before any conversion
 *  4 ok &= the target pixel (vi, ui) has a normal;  M = P1(vi, ui), n its normal
 *  5 if pairs[t - 1] != 0:  ok &= L1(vi, ui) == pairs[t - 1]
 *  6 d = Q - M;   ok &= pdot(d, d) <= dist_max * dist_max;   r = pdot(n, d);   ok &= fabsf(r) <= dist_max
 *  7 J = (pcross(Q, n), n), quantised as in sf_align.h:
 *      a_k = (int64)rintf(fminf(fmaxf(J_k, -64.f), 64.f) * 4096.f)          rho = (int64)rintf(r * 65536.f)
 *  8 the system is an sfb_system, the system record of sf_align.h field for field: n = number of ok pixels,
 *    ss = sum rho * rho, g[k] = sum a_k * rho, H[.] = sum a_k * a_l for k <= l row-wise, reserved words 0.
 *    The bounds of sf_align.h hold (at most 2^24 pixels), and integer sums make a system a function of the inputs alone,
 *    for any batch composition and from run to run.
 *    In metres: rms point-to-plane residual = sqrt(ss / n) / 65536.
 *
 * LOOP, per region, exactly the LOOP of sf_align.h with the parameters iterations, min_pairs and damping and the STEP
 * of sf_align.h (the same program text): for it = 0 .. iterations - 1: linearise at D (system `it`); if n < min_pairs stop with
 * SFB_FEW_PAIRS; take the step; if it is refused stop with SFB_DEGENERATE; else D = D_out. After the loop one more
 * linearisation at the returned D (system `iterations`) gives n_last and ss_last. On a stop D is the one before the refused
 * step, the stopping linearisation was taken at it and n_last, ss_last are its n and ss; iterations_done counts the steps
 * taken. Regions of one entry stop independently. n_first, ss_first are n and ss of system 0: ss_first / n_first is the
 * misfit of the "did not move" hypothesis, the quantity a caller thresholds.
 *
 * WORLD MOTION.  W = (T1 * D) * T0^-1 takes a world point of the body at time 0 to its place at time 1. With
 * T0[r][c] = (double)C0.pose[r + 4 * c], T1 likewise, in fp64 in the written order, only + - * /, T0^-1 formed by the
 * transpose as the relative transform of sf_tracks.h forms it:
 *   A[r][c] = (T1[r][0] * D[0][c] + T1[r][1] * D[1][c]) + T1[r][2] * D[2][c],   and for c == 3 that sum + T1[r][3]     r < 3
 *   W[r][c] = (A[r][0] * T0[c][0] + A[r][1] * T0[c][1]) + A[r][2] * T0[c][2]                                        r, c < 3
 *   W[r][3] = A[r][3] - ((W[r][0] * T0[0][3] + W[r][1] * T0[1][3]) + W[r][2] * T0[2][3])       (the unrounded W[r][c])
 *   w[r + 4 * c] = (float)W[r][c], each entry rounded once; w[3], w[7], w[11] = 0, w[15] = 1.
 * A region that did not move gives W = I up to the rounding of D0 and of the products.
 *
 * RESULT.  One sfb_motion per (entry, region slot), M per entry, entry q's at q * M; records K .. M - 1 are written as zeros.
 * d is D as a column-major 4 x 4, d[k + 4 * c] = (float)D[k][c] with last row 0 0 0 1; w is the world motion of that D.
 * systems_out is NULL or room for n * M * (I + 1) records of sfb_system, I the largest `iterations` of the call: record
 * (q * M + t - 1) * (I + 1) + it is system `it` of region t of entry q; records after a region's last linearisation (a stop,
 * or fewer iterations than I) and those of slots K .. M - 1 are zeros.
 *
 * All functions return SF_OK or the SF_ERR_* codes of sf.h; sf_last_error() has the text.
 *
 * REFUSALS (SF_ERR_ARG unless said otherwise; nothing launched, nothing written): a null argument (labels1, pairs and
 * systems_out may be NULL, and so may single entries of labels1); n < 0 or n > 65535 (n == 0 is SF_OK); rows or cols outside
 * 1..4096 or rows * cols > 2^24; max_regions outside 1..256; an n_regions entry outside 0..max_regions; a pair entry < 0; a
 * non-zero pair among the first n_regions of an entry whose L1 is missing; a non-finite camera entry, or fx or fy equal to 0;
 * a NaN or inf in sfb_params; dist_max outside (0, 1]; z_max outside (0, 32]; normal_dz outside (0, 32]; a negative damping;
 * iterations outside 1..64; min_pairs < 6; a handle that has been destroyed (SF_ERR_STATE); scratch that cannot be grown (the
 * allocation's own code).
 *
 * NOT HERE: photometric terms, robust weights beyond the gates, image pyramids and large inter-frame motions, motion priors
 * carried from the previous frame, a per-region initial estimate, fusing a body into a map of its own, a stream or tracker
 * form (neither keeps a previous label image a reader may use), and checkpointing.
 */
#ifndef SF_BODIES_H_
#define SF_BODIES_H_

#include "sf_align.h"
#include "sf_tracks.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the values of the status codes of sf_align.h */
#define SFB_OK 0
#define SFB_FEW_PAIRS 1
#define SFB_DEGENERATE 2

/* The camera of sf_tracks.h and the system record of sf_align.h under names of this interface: the same fields at the same
 * offsets, so that a record of either header can be handed to the other as it is. (Every companion header keeps its
 * prefix to itself; the library asserts that the layouts agree.) */
typedef struct sfb_camera {
    float pose[16];        /* camera-to-world, column-major */
    float cx, cy, fx, fy;  /* pixels; fx, fy != 0 */
} sfb_camera;              /* 80 bytes; sfb_camera_bytes() reports it */

typedef struct sfb_system {
    int64_t n, ss;
    int64_t g[6];
    int64_t H[21];
    int64_t reserved[3];  /* written as 0 */
} sfb_system;             /* 256 bytes; sfb_system_bytes() reports it */

typedef struct sfb_params {
    float   dist_max;    /* metres, 0 < . <= 1: gate on |Q - M| and on |r| */
    float   z_max;       /* metres, 0 < . <= 32: depths beyond it are not used, in either frame */
    float   normal_dz;   /* metres, 0 < . <= 32: the largest depth step to a neighbour a normal is taken across */
    float   damping;     /* >= 0: damping * n is added to the diagonal of A */
    int32_t iterations;  /* 1..64 */
    int32_t min_pairs;   /* >= 6 */
    int32_t reserved[2]; /* not read */
} sfb_params;            /* 32 bytes; sfb_params_bytes() reports it */

typedef struct sfb_motion {
    float   d[16];        /* D, column-major 4 x 4 */
    float   w[16];        /* W = (T1 * D) * T0^-1, column-major 4 x 4 */
    int32_t status;       /* SFB_OK, SFB_FEW_PAIRS, SFB_DEGENERATE */
    int32_t iterations_done;
    int64_t n_first, ss_first, n_last, ss_last;
    int64_t reserved[3];  /* written as 0 */
} sfb_motion;             /* 192 bytes; sfb_motion_bytes() reports it */

int sfb_version(void); /* 1 */
size_t sfb_params_bytes(void); /* 32 */
size_t sfb_motion_bytes(void); /* 192 */
size_t sfb_camera_bytes(void); /* 80 */
size_t sfb_system_bytes(void); /* 256 */

/* dist_max 0.10, z_max 8, normal_dz 0.05, damping 0, iterations 10, min_pairs 64. These are parameter defaults, NOT tuned
 * values: nobody has tuned them on real data, and whether a motion is good enough (n_last, ss_last against n_first, ss_first)
 * is the caller's to decide. */
int sfb_default_params(sfb_params *p);

/* Pure host, no handle, no GPU: SF_OK, or SF_ERR_ARG for null parameters or ones the refusal list names. */
int sfb_check_params(const sfb_params *p);

/* Pure host, no handle, no GPU: WORLD MOTION as stated above (the device compiles the same text). pose0 and pose1 are
 * camera-to-world, column-major; D is row-major 3 x 4. SF_ERR_ARG for a null argument or a NaN or inf in any input. */
int sfb_world_motion(const float pose0[16], const float pose1[16], const double D[12], float w_out[16]);

/* Entry q < n aligns the regions of frame 0 with frame 1. depth0, labels0, depth1 are arrays of n HOST pointers to rows x cols
 * images; labels1 is NULL or such an array, whose entries may be NULL; cams0, cams1 and params hold n entries, n_regions n
 * counts; pairs is NULL or n * max_regions int32. motions_out is HOST memory for n * max_regions records, systems_out NULL
 * or HOST memory as stated above. Ordered on the handle's HIP stream; returns after the results are in host memory. */
int sfb_estimate_images(sf_handle *h, int rows, int cols, int n, const float *const *depth0, const int32_t *const *labels0, const float *const *depth1,
                        const int32_t *const *labels1, const sfb_camera *cams0, const sfb_camera *cams1, const int32_t *n_regions, const int32_t *pairs,
                        const sfb_params *params, int max_regions, sfb_motion *motions_out, sfb_system *systems_out);

/* The same with DEVICE pointers in the (host) arrays depth0, labels0, depth1 and labels1 -- the label images are what
 * sfr_label_images_device wrote, the depths the caller's buffers: a device-resident pipeline keeps two generations of
 * each --; motions_out is ONE device pointer to n * max_regions records, systems_out NULL or ONE device pointer to
 * n * max_regions * (I + 1) records, 8-byte aligned. Asynchronous on the handle's stream; nothing is read back. */
int sfb_estimate_images_device(sf_handle *h, int rows, int cols, int n, const void *const *depth0, const void *const *labels0, const void *const *depth1,
                               const void *const *labels1, const sfb_camera *cams0, const sfb_camera *cams1, const int32_t *n_regions, const int32_t *pairs,
                               const sfb_params *params, int max_regions, void *motions_out, void *systems_out);

#ifdef __cplusplus
}
#endif
#endif
