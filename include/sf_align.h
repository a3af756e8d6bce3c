/* sf_align.h — refine poses against a map: damped point-to-plane steps with integer normal equations.
 *
 * A companion of sf.h, not part of its ABI: plain C declarations with the prefix sfa_, exported by libsf_hip.so (and its
 * precise and reference-order builds) only. The CPU oracle does not implement them and SF_ABI_VERSION does not count them;
 * sfa_version() versions this interface.
 *
 * sfk_query_* proposes the pose of an earlier keyframe and sfs_score_* ranks such candidates; neither is the pose of this
 * frame. These calls refine many (map, candidate pose, frame) triples per call -- the same map and the same frame any
 * number of times -- on the device, without a host synchronisation between iterations. A refine call only READS its maps and
 * streams: afterwards the map, sf_map_info, sf_map_get_index_map, the predictions, the streams, the view scratch,
 * sfv_last_large_sprites and the scratch of the score and region calls are what they were. Nothing is written back into a
 * stream or a map: what to do with a refined pose is the caller's to decide.
 *
 * THE MAP of an entry is drawn ONCE from view.pose = T0, the candidate pose, exactly as sf_view.h and sf_score.h draw it
 * (same culls, sprites, fragment test and 64-bit (depth, index) minimum; view.shade must be valid and is otherwise ignored).
 * For a DRAWN pixel (i, j) (column i, row j) with winner s, let h, n be the camera-frame position and normalised normal of s
 * (sf_view.h), l the view ray of the pixel, normalize((i + 0.5 - cx) / fx, (j + 0.5 - cy) / fy, 1), and
 *   pdot(a, b) = (a.x * b.x + a.y * b.y) + a.z * b.z
 *   t = pdot(h, n) / pdot(l, n)          M = (l.x * t, l.y * t, l.z * t)        (M.z is the zm of a score)
 *
 * THE FRAME is a depth image zf and with use_b a b image, both of the view's size, column-major float32 like every image
 * of sf.h: element (y, x) at y + x * rows. It was taken with the view's intrinsics.
 *
 * THE ESTIMATE is a 3 x 4 matrix D, row-major D[k][c] = D[4 * k + c], that maps the frame's camera into T0's camera. It is
 * carried in fp64, used by the pixel pass rounded to float, and starts as D0 = I.
 *
 * LINEARISATION at D. All arithmetic fp32 in the written order without contraction; a comparison with a NaN operand is
 * false. Over the frame pixels (y, x) with x % stride == 0 && y % stride == 0:
 *   ok  = zf > 0 && zf <= z_max && (use_b ? b > b_min : true)
 *   P   = ( (((float)x - cx) * zf) / fx,  (((float)y - cy) * zf) / fy,  zf )
 *   Q.k = ((D[k][0] * P.x + D[k][1] * P.y) + D[k][2] * P.z) + D[k][3]            ok &= Q.z >= 0.4f
 *   px  = (fx * Q.x) / Q.z + cx          py = (fy * Q.y) / Q.z + cy
 *   ok &= px >= 0 && px < (float)cols && py >= 0 && py < (float)rows             i = (int)floorf(px), j = (int)floorf(py)
 *   ok &= pixel (i, j) is drawn;         M, n of that pixel
 *   d   = Q - M                          ok &= pdot(d, d) <= dist_max * dist_max
 *                                        ok &= pdot(n, n) > 0.5f
 *   r   = pdot(n, d)                     ok &= fabsf(r) <= dist_max
 *   c   = (Q.y * n.z - n.y * Q.z,  Q.z * n.x - n.z * Q.x,  Q.x * n.y - n.x * Q.y)        J = (c.x, c.y, c.z, n.x, n.y, n.z)
 *   a_k = (int64)rintf(fminf(fmaxf(J_k, -64.f), 64.f) * 4096.f)                  rho = (int64)rintf(r * 65536.f)
 * P uses the fusion's pixel convention (pixel centres at integers: that is how the surfels were made); the drawn view keeps
 * the half pixel of gl_FragCoord. The two are not unified on purpose. The system of a linearisation is sfa_system:
 *   n = number of ok pixels,  ss = sum rho * rho,  g[k] = sum a_k * rho,  H[.] = sum a_k * a_l for k <= l, row-wise
 *   (H[0] = 00, 01, .. 05, 11, 12, .. 55 = H[20]), three reserved words written as 0.
 * |a| <= 2^18, |rho| <= 2^16 and at most 2^24 pixels: every sum stays below 2^61. Integer sums do not depend on the order
 * of summation: a system is a function of its inputs alone, for any batch composition and from run to run.
 * In metres: rms point-to-plane residual = sqrt(ss / n) / 65536.
 *
 * STEP (sfa_step; the device runs the same text). fp64 in the written order without contraction, only + - * /:
 *   A[k][l] = A[l][k] = (double)H_kl * 2^-24,  then A[k][k] += (double)damping * (double)n;     b[k] = -((double)g[k] * 2^-28)
 *   LDL^T without pivoting, for j = 0..5:
 *     d[j] = A[j][j] - sum_{k<j} (L[j][k] * L[j][k]) * d[k]          (the sum subtracted term by term, ascending k)
 *     if !(d[j] > 1e-9 * (double)n) the step is refused: SFA_DEGENERATE, D_out is not written
 *     L[i][j] = (A[i][j] - sum_{k<j} (L[i][k] * L[j][k]) * d[k]) / d[j]   for i > j
 *   z[i] = b[i] - sum_{k<i} L[i][k] * z[k];   y[i] = z[i] / d[i];   x[i] = y[i] - sum_{k>i} L[k][i] * x[k] (i = 5..0, ascending k)
 *   xi = x = (w0, w1, w2, u0, u1, u2).  The rotation is the Cayley map of w, no sin, cos or sqrt:
 *     a = 0.5 * w,  aa = (a0 * a0 + a1 * a1) + a2 * a2,  s = 2 / (1 + aa)
 *     R00 = 1 - s * (a1 * a1 + a2 * a2)   R01 = s * (a0 * a1 - a2)            R02 = s * (a0 * a2 + a1)
 *     R10 = s * (a0 * a1 + a2)            R11 = 1 - s * (a0 * a0 + a2 * a2)   R12 = s * (a1 * a2 - a0)
 *     R20 = s * (a0 * a2 - a1)            R21 = s * (a1 * a2 + a0)            R22 = 1 - s * (a0 * a0 + a1 * a1)
 *   D_out[k][c] = (R[k][0] * D[0][c] + R[k][1] * D[1][c]) + R[k][2] * D[2][c],  and for c == 3 that sum + u_k.
 *
 * LOOP, per entry, for it = 0 .. iterations - 1: linearise at D (system `it`); if n < min_pairs stop with SFA_FEW_PAIRS;
 * take the step; if it is refused stop with SFA_DEGENERATE; else D = D_out. After the loop one more linearisation at the
 * returned D (system `iterations`) gives n_last and ss_last. On a stop D is the one before the refused step, the stopping
 * linearisation was taken at it and n_last, ss_last are its n and ss; iterations_done counts the steps taken.
 *   pose = T0 * D in fp64, pose[r + 4 * c] = (float)((T0[r][0] * D[0][c] + T0[r][1] * D[1][c]) + T0[r][2] * D[2][c]) and for
 *   c == 3 that sum + T0[r][3] before the rounding, r = 0..3, T0[r][c] = (double)view.pose[r + 4 * c].
 *
 * systems_out is NULL or room for n * (I + 1) records, I the largest `iterations` of the call: record q * (I + 1) + it is
 * system `it` of entry q; records after an entry's last linearisation (a stop, or fewer iterations than I) are zeros.
 *
 * All functions return SF_OK or the SF_ERR_* codes of sf.h (sfa_step: its status); sf_last_error() has the text.
 *
 * REFUSALS (SF_ERR_ARG unless said otherwise; nothing launched, nothing written): a null argument (systems_out and b may
 * be NULL); n < 0 (n == 0 is SF_OK); n > 65535; a map of another handle; a map whose handle was destroyed (SF_ERR_STATE);
 * every refusal of sfv_check_view; a stream index out of range (the code of sf_get_current); a view whose rows and cols are
 * not the handle's in the stream form; a NaN or inf in sfa_params; dist_max outside (0, 1]; z_max outside (0, 32]; a negative
 * damping; iterations outside 1..64; stride outside 1..16; min_pairs < 6; use_b other than 0 / 1; a null depth image;
 * use_b with its image missing; scratch that cannot be allocated (SF_ERR_NOMEM).
 *
 * OUT OF SCOPE: photometric terms, frame normals, robust weights beyond the gate, image pyramids, and writing the refined
 * pose back into a stream or a map.
 */
#ifndef SF_ALIGN_H_
#define SF_ALIGN_H_

#include "sf_view.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SFA_OK 0
#define SFA_FEW_PAIRS 1
#define SFA_DEGENERATE 2

typedef struct sfa_params {
    float   dist_max;    /* metres, 0 < . <= 1: gate on |Q - M| and on |r| */
    float   z_max;       /* metres, 0 < . <= 32: frame depths beyond it are not used */
    float   b_min;       /* with use_b: a frame pixel counts when b > b_min */
    float   damping;     /* >= 0: damping * n is added to the diagonal of A */
    int32_t iterations;  /* 1..64 */
    int32_t stride;      /* 1..16: every stride-th row and column of the frame */
    int32_t min_pairs;   /* >= 6 */
    int32_t use_b;       /* 0 / 1 */
} sfa_params;            /* 32 bytes; sfa_params_bytes() reports it */

typedef struct sfa_system {
    int64_t n, ss;
    int64_t g[6];
    int64_t H[21];
    int64_t reserved[3];  /* written as 0 */
} sfa_system;             /* 256 bytes; sfa_system_bytes() reports it */

typedef struct sfa_result {
    float   pose[16];     /* T0 * D, column-major */
    int32_t status;       /* SFA_OK, SFA_FEW_PAIRS, SFA_DEGENERATE */
    int32_t iterations_done;
    int64_t n_first, ss_first, n_last, ss_last;
    int64_t reserved[3];  /* written as 0 */
} sfa_result;             /* 128 bytes; sfa_result_bytes() reports it */

int sfa_version(void); /* 1 */
size_t sfa_params_bytes(void); /* sizeof(sfa_params) = 32 */
size_t sfa_result_bytes(void); /* sizeof(sfa_result) = 128 */
size_t sfa_system_bytes(void); /* sizeof(sfa_system) = 256 */

/* dist_max 0.15, z_max 8, b_min 0.5, damping 0, iterations 10, stride 1, min_pairs 64, use_b 1. These are parameter
 * defaults, NOT tuned values: nobody has tuned them on real data, and whether a result is good enough (n_last, ss_last, a
 * score of the refined pose) is the caller's to decide. */
int sfa_default_params(sfa_params *p);

/* Pure host, no handle, no GPU: SF_OK, or SF_ERR_ARG for null parameters or ones the refusal list names. */
int sfa_check_params(const sfa_params *p);

/* Pure host, no handle, no GPU: one STEP as stated above. SFA_OK and D_out written, SFA_DEGENERATE and D_out untouched, or
 * SF_ERR_ARG for a null argument. D_in and D_out may be the same array. */
int sfa_step(const sfa_system *s, float damping, const double D_in[12], double D_out[12]);

/* Entry q < n refines views[q].pose against maps[q] with the current frame of streams[q]: the level-0 depth sf_get_current
 * returns and, with use_b, the image sf_get_b_image returns, read on the device where they lie. The rows and cols of
 * views[q] must be the handle's. params and views hold n entries, results is HOST memory for n records, systems_out NULL or
 * HOST memory as stated above. Ordered on the handle's HIP stream; returns after the results are in host memory. */
int sfa_refine_streams(sf_handle *h, int n, sf_map *const *maps, const sfv_view *views, const int32_t *streams, const sfa_params *params,
                       sfa_result *results, sfa_system *systems_out);

/* The same with frames in HOST memory: depth[q] (and b[q]) of the size of views[q], 1 to 4096 rows and columns, column-major
 * float32 -- the output of sf_get_current goes straight in. b is an array of n pointers, or NULL; use_b set in params[q] with
 * its pointer missing is SF_ERR_ARG, a pointer whose flag is clear is not read. */
int sfa_refine_images(sf_handle *h, int n, sf_map *const *maps, const sfv_view *views, const float *const *depth, const float *const *b,
                      const sfa_params *params, sfa_result *results, sfa_system *systems_out);

/* The same with DEVICE pointers in the (host) arrays depth and b; results is ONE device pointer to n records, systems_out
 * NULL or ONE device pointer to n * (I + 1) records. Asynchronous on the handle's stream; nothing is read back. */
int sfa_refine_images_device(sf_handle *h, int n, sf_map *const *maps, const sfv_view *views, const void *const *depth, const void *const *b,
                             const sfa_params *params, void *results, void *systems_out);

#ifdef __cplusplus
}
#endif
#endif
