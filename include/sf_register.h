/* sf_register.h — register surfel maps against each other on a voxel table: map-to-map point-to-plane alignment.
 *
 * A companion of sf.h, not part of its ABI: plain C declarations with the prefix sfg_, exported by libsf_hip.so (and its
 * precise and reference-order builds) only. The CPU oracle does not implement them and SF_ABI_VERSION does not count them;
 * sfg_version() versions this interface.
 *
 * The library can cull, thin, merge, bend, carve and draw surfel maps and refine a FRAME against a map; every call that puts two
 * MAPS into one frame (the merge of sf_join.h, the body maps of sf_body_maps.h after a body comes back into view, the two
 * parts of a map after a deformation of sf_deform.h, two sessions that saw one room) takes its 4 x 4 transform from outside.
 * These calls estimate it from the two maps alone: many (destination, source, start) entries per call, each refined on the
 * device by damped point-to-plane steps whose partners come from a voxel table of the destination, without a host
 * synchronisation between iterations. Both maps of an entry are only READ: afterwards the maps, sf_map_info and
 * sf_map_get_index_map are what they were. What to do with a result is the caller's to decide.
 *
 * DEFINITIONS. s[0..11] is a surfel in the layout of sf.h (position + confidence; colour, -, init time, last time; normal +
 * radius). All surfel-level arithmetic is fp32, one rounding per operation written, without contraction; a comparison with a
 * NaN operand is false.   pdot(a, b) = (a.x * b.x + a.y * b.y) + a.z * b.z
 *
 * TABLE. The table of a destination map for a `cell` is exactly the thin table of sf_join.h: the same key, grid limits, rank,
 * slot count, hash and linear probing. The REPRESENTATIVE of an occupied voxel is the surfel of highest rank, among equal
 * ranks the one of lowest index. Destination surfels outside the grid occupy nothing. Entries of one call that name the same
 * destination with the same cell share one table; a table is a set, so no result depends on that.
 *
 * ESTIMATE. E is 3 x 4, row-major E[4 * k + c], from the source's world frame to the destination's. It is carried in fp64 and
 * used by the surfel pass rounded to float. It starts as E0[k][c] = (double)T0[k + 4 * c]; T0 is column-major 4 x 4 (its last row
 * is not read). A null T0 means identities, and the same arithmetic runs.
 *
 * SAMPLE. The source surfels e with e % stride == 0; with min_confidence > 0 of those only the ones with s[3] >= min_confidence.
 *
 * PAIR of a sampled source surfel with position p and normal m at E:
 *   Q.k  = ((E[k][0] * p.x + E[k][1] * p.y) + E[k][2] * p.z) + E[k][3]        m'.k the same without the last term
 *   sc_i = Q_i * inv,  inv = 1.0f / cell evaluated once, on the host          f_i = floorf(sc_i)
 *   Q is OUTSIDE THE GRID by the rule of sf_join.h (a Q_i or f_i that is not finite, or |f_i| >= 2^20): the surfel is counted in
 *   n_outside and is not paired. Otherwise, per axis,
 *   side_i = (sc_i - f_i < 0.5f) ? -1 : +1
 *   and the 2 x 2 x 2 NEIGHBOURHOOD is the eight voxels (f_x + a * side_x, f_y + b * side_y, f_z + c * side_z), a, b, c in {0, 1},
 *   visited with a outermost and c innermost; a neighbour whose index leaves the grid is skipped. For every visited voxel that
 *   is occupied, with its representative at position M:   d = Q - M,   dd = pdot(d, d).
 *   The PARTNER is the representative with the smallest dd; a later one replaces an earlier one only when its dd is strictly
 *   smaller. The gates, in this order:
 *     1. a partner exists;
 *     2. with min_confidence > 0: the partner's s[3] >= min_confidence;
 *     3. dd <= dist_max * dist_max;
 *     4. n = v / sqrtf(pdot(v, v)) of the partner's normal v exists: 0 < pdot(v, v) < INFINITY (the rule of sf_deform.h), each
 *        component divided by the root;
 *     5. the same for m', giving mn;
 *     6. pdot(mn, n) >= min_cos;
 *     7. r = pdot(n, d) and fabsf(r) <= dist_max.
 *   dist_max <= 0.5f * cell is required, so every representative within dist_max of Q lies in the neighbourhood.
 *   The row is that of sf_align.h with this Q, n and r:
 *   c   = (Q.y * n.z - n.y * Q.z,  Q.z * n.x - n.z * Q.x,  Q.x * n.y - n.x * Q.y)        J = (c.x, c.y, c.z, n.x, n.y, n.z)
 *   a_k = (int64)rintf(fminf(fmaxf(J_k, -64.f), 64.f) * 4096.f)                  rho = (int64)rintf(r * 65536.f)
 * The system of a linearisation is sfg_system, word for word the system of sf_align.h:
 *   n = number of pairs,  ss = sum rho * rho,  g[k] = sum a_k * rho,  H[.] = sum a_k * a_l for k <= l, row-wise
 *   (H[0] = 00, 01, .. 05, 11, 12, .. 55 = H[20]), three reserved words written as 0.
 * |a| <= 2^18, |rho| <= 2^16 and at most 2^24 sampled surfels per entry: every sum stays below 2^61. Integer sums do not depend
 * on the order of summation: a system is a function of its inputs alone, for any batch composition and from run to run.
 * In metres: rms point-to-plane residual = sqrt(ss / n) / 65536.
 *
 * STEP. The step of sf_align.h applies to these words unchanged (fp64, only + - * /, LDL^T without pivoting, the Cayley map),
 * with E for D: E_out = [R | u] * E, or the step is refused.
 *
 * LOOP, per entry, for it = 0 .. iterations - 1: linearise at E (system `it`); if n < min_pairs stop with SFG_FEW_PAIRS; take
 * the step; if it is refused stop with SFG_DEGENERATE; else E = E_out. After the loop one more linearisation at the returned E
 * (system `iterations`) gives n_last, ss_last, n_sampled, n_outside and, where asked for, the pairs. On a stop E is the one
 * before the refused step, the stopping linearisation was taken at it and n_last, ss_last, the two counts and the pairs are
 * its; iterations_done counts the steps taken. T of the result is E rounded to float, column-major, with last row 0 0 0 1.
 *
 * systems_out is NULL or room for n * (I + 1) records, I the largest `iterations` of the call: record q * (I + 1) + it is
 * system `it` of entry q; records after an entry's last linearisation (a stop, or fewer iterations than I) are zeros.
 * pairs_out is NULL or n pointers, each NULL or room for the count of the entry's source in int32: at the last linearisation
 * the partner's index in the destination, -1 for a sampled surfel that is not paired, -2 for one that is not sampled.
 *
 * WHY THIS RULE. The eight voxels on Q's side of its cell hold every point within cell / 2 of Q, so with dist_max <= cell / 2
 * the search misses no representative the gate would have let through, at a fixed cost of eight probes. The partner is the
 * REPRESENTATIVE of a voxel and not the nearest surfel because the thin table of sf_join.h already holds it: one table, one
 * insert kernel, and a pair costs eight probes and two gathers however dense the destination is. The price: the nearest surfel
 * of the destination may be another one of the same voxel, so in a dense map the point-to-plane residual is taken against a
 * surfel up to a cell away along the surface; its plane is what the residual measures, and a smaller cell buys accuracy.
 *
 * All functions return SF_OK or the SF_ERR_* codes of sf.h; sf_last_error() has the text. sfg_register_maps is ordered on the
 * handle's HIP stream and returns after the results are in host memory. One set of launches serves the whole batch. A call
 * needs 16 bytes of registrar scratch per slot of a distinct table, 4 per destination surfel, 256 per system record and, where
 * pairs are asked for, 4 per sampled surfel; the scratch grows with the largest call and is freed with the registrar.
 *
 * REFUSALS (SF_ERR_ARG unless said otherwise; nothing launched, nothing written): a null argument where one is needed (T0,
 * systems_out and pairs_out may be NULL); n < 0 (n == 0 is SF_OK) or n > 65535; a map of another handle than the registrar's;
 * a registrar or a map whose handle was destroyed (SF_ERR_STATE); dst[q] == src[q]; a non-finite entry of T0; a cell that is not
 * finite or not > 0 or whose 1.0f / cell is not finite; dist_max outside (0, 1] or > 0.5f * cell; min_cos outside [-1, 1]; a NaN
 * min_confidence; a negative or non-finite damping; iterations outside 1..64; stride < 1; min_pairs < 6; more than 2^24 surfels
 * e % stride == 0 in a source; scratch that cannot be grown (the allocation's own code). A probe walk that visits every slot
 * without finding its key or an empty slot sets the entry's error word and the call returns SF_ERR_STATE with nothing written; at
 * a load of one half that cannot happen, and every loop is bounded so that it cannot hang either. An empty destination or
 * source is not refused: the entry ends SFG_FEW_PAIRS at iteration 0.
 *
 * OUT OF SCOPE: colour terms; robust weights beyond the gates; a global search (without an initial guess); multi-resolution
 * tables; writing T into a map, a stream or a merge; a device-pointer form; symmetric pairing (both directions).
 */
#ifndef SF_REGISTER_H_
#define SF_REGISTER_H_

#include "sf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SFG_OK 0
#define SFG_FEW_PAIRS 1
#define SFG_DEGENERATE 2

typedef struct sfg_params {
    float   cell;           /* edge of a voxel in metres: finite, > 0, and 1.0f / cell finite */
    float   dist_max;       /* metres, 0 < . <= 1 and <= 0.5f * cell: gate on |Q - M| and on |r| */
    float   min_cos;        /* -1 <= . <= 1: gate on the cosine between the moved source normal and the partner's */
    float   min_confidence; /* enabled when > 0: source surfels and partners with s[3] >= min_confidence only; not NaN */
    float   damping;        /* >= 0, finite: damping * n is added to the diagonal of A */
    int32_t iterations;     /* 1..64 */
    int32_t stride;         /* >= 1: every stride-th surfel of the source */
    int32_t min_pairs;      /* >= 6 */
} sfg_params;               /* 32 bytes; sfg_params_bytes() reports it */

typedef struct sfg_system {
    int64_t n, ss;
    int64_t g[6];
    int64_t H[21];
    int64_t reserved[3];  /* written as 0 */
} sfg_system;             /* 256 bytes; sfg_system_bytes() reports it */

typedef struct sfg_result {
    float   T[16];        /* E rounded to float, column-major, last row 0 0 0 1 */
    int32_t status;       /* SFG_OK, SFG_FEW_PAIRS, SFG_DEGENERATE */
    int32_t iterations_done;
    int64_t n_first, ss_first, n_last, ss_last;
    int32_t n_sampled;    /* at the last linearisation: the sampled surfels */
    int32_t n_outside;    /* ... and of those, the ones whose Q is outside the grid */
    int32_t reserved[4];  /* written as 0 */
} sfg_result;             /* 128 bytes; sfg_result_bytes() reports it */

typedef struct sfg_registrar sfg_registrar;

int sfg_version(void); /* 1 */
size_t sfg_params_bytes(void); /* sizeof(sfg_params) = 32 */
size_t sfg_system_bytes(void); /* sizeof(sfg_system) = 256 */
size_t sfg_result_bytes(void); /* sizeof(sfg_result) = 128 */

/* cell 0.1, dist_max 0.05, min_cos 0.5, min_confidence 0, damping 0, iterations 10, stride 1, min_pairs 64.
 * These are parameter defaults, NOT tuned values: nobody has tuned them on real data, and whether a result is good enough
 * (n_last, ss_last, a dry-run merge with T) is the caller's to decide. */
int sfg_default_params(sfg_params *p);

/* Pure host, no handle, no GPU: SF_OK, or SF_ERR_ARG for null parameters or ones the refusal list names. */
int sfg_check_params(const sfg_params *p);

/* Pure host, no handle, no GPU: one linearisation of src (src_count surfels of 12 floats) against the table of dst (dst_count
 * surfels) at the estimate E, the table built sequentially in host memory, the rule text the device runs. system_out is
 * written; pairs_out is NULL or room for src_count values as stated above. iterations, damping and min_pairs are checked and not
 * used. SF_ERR_ARG for a null argument where a count is not 0, a negative count or one above 2^29, a non-finite E, bad
 * parameters or more than 2^24 surfels e % stride == 0. */
int sfg_linearise(const float *dst, int dst_count, const float *src, int src_count, const sfg_params *params, const double E[12],
                  sfg_system *system_out, int32_t *pairs_out);

/* A registrar holds the scratch of the register calls made through it. It belongs to h; when h is destroyed first it releases
 * the memory and every call but sfg_registrar_destroy answers SF_ERR_STATE. */
int sfg_registrar_create(sf_handle *h, sfg_registrar **out);
void sfg_registrar_destroy(sfg_registrar *reg);

/* Entry q < n registers src[q] against dst[q] from T0 + 16 q (T0 null: n identities) with params[q]. The maps belong to the
 * registrar's handle. results is HOST memory for n records, systems_out and pairs_out NULL or HOST memory as stated above. */
int sfg_register_maps(sfg_registrar *reg, int n, sf_map *const *dst, sf_map *const *src, const float *T0, const sfg_params *params,
                      sfg_result *results, sfg_system *systems_out, int32_t *const *pairs_out);

#ifdef __cplusplus
}
#endif
#endif
