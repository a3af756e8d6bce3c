/* sf_deform.h — bend surfel maps with a deformation graph: bind, solve, apply.
 *
 * A companion of sf.h, not part of its ABI: plain C declarations with the prefix sfd_, exported by libsf_hip.so (and its
 * precise and reference-order builds) only. The CPU oracle does not implement them and SF_ABI_VERSION does not count them;
 * sfd_version() versions this interface.
 *
 * When a stream comes back to a place after a long walk, the pose refined against the map (sf_align.h) and the drifted pose
 * disagree, and the disagreement is not rigid: the drift is spread over the whole loop. One transform (the merge of
 * sf_join.h, the move of sf_body_maps.h) either tears the map where the loop began or leaves a doubled wall where it ends.
 * A DEFORMATION GRAPH spreads the correction: a few hundred nodes sampled from the map, each with a rigid transform of its
 * own; every surfel follows the nodes near it in space and in time. This is the deformation graph of ElasticFusion
 * (Whelan et al., RSS 2015) after Sumner et al., Embedded Deformation for Shape Manipulation (SIGGRAPH 2007).
 *
 * DEFINITIONS. s[0..11] is a surfel in the layout of sf.h (position + confidence; colour, weight, init time, last time;
 * normal + radius). Unless said otherwise all arithmetic is fp32, one rounding per operation in the written order, without
 * contraction; a comparison with a NaN operand is false.
 *
 * NODE j < G. A node has a position g_j (3 floats), a time_j (float) and a transform M_j, a row-major 3 x 4 matrix [A | t]:
 * A[r][c] = M[4 r + c], t.r = M[4 r + 3]. The identity with t = 0 means "does not move". G <= SFD_MAX_NODES = 1024.
 * A node moves a point as
 *   phi_j(p).r = (((A[r][0]*d.x + A[r][1]*d.y) + A[r][2]*d.z) + g.r) + t.r        with d = p - g_j
 * and a direction as (A n).r = (A[r][0]*n.x + A[r][1]*n.y) + A[r][2]*n.z.
 *
 * BIND of a point p with time tau (the rule of ElasticFusion, without its temporal pre-sort):
 *   dx = p.x - g_j.x, likewise dy, dz;   d2_j = (dx*dx + dy*dy) + dz*dz
 *   Node j is ELIGIBLE when d2_j < INFINITY and fabsf(time_j - tau) <= time_window hold. With an infinite window and a finite
 *   tau that admits every node whose time is not NaN.
 *   The E eligible nodes are ordered by (d2, j) ascending; the first m = min(4, E) are taken, i = 0 .. m - 1.
 *   dmax2 is the d2 of the fifth node when E > 4, and otherwise 4.0f * the d2 of the m-th.
 *   w_i = 1.0f - sqrtf(d2_i) / sqrtf(dmax2), then w_i = w_i * w_i. When dmax2 == 0, every w_i = 1.
 *   S = ((w_0 + w_1) + w_2) + w_3 over the taken nodes. When !(S > 0), every w_i = 1 and S = (float)m.
 *   The weights are w_i / S. A binding is written as 4 indices and 4 weights; a missing index is -1, a missing weight 0.
 *   E == 0 means UNBOUND.
 *
 * DEFORM of a surfel s. It is bound with p = s[0..2] and tau = s[6] (the init time). Bound to m nodes:
 *   the position becomes, per coordinate r, the ascending-i sum of w_i * phi_i(p).r, starting from the first term;
 *   the normal n = s[8..10] becomes the ascending-i sum of w_i * (A_i n).r, then divided by sqrtf(nn),
 *   nn = (n.x*n.x + n.y*n.y) + n.z*n.z of the sum, when nn > 0 && nn < INFINITY holds; otherwise the old normal stays (the
 *   rule of the merge in sf_body_maps.h);
 *   s[3..7] and s[11] stay bit for bit.
 * An UNBOUND surfel stays bit for bit and is counted.
 *
 * EDGES of node j: BIND of g_j with tau = time_j over the OTHER nodes; the first min(4, E) indices are the edges, a missing
 * one is -1.
 *
 * POSE. A pose is a column-major 4 x 4 like every pose of sf.h, with a time tau. Its origin (elements 12..14) is bound with tau
 * and deformed as a position; the three axes a_0, a_1, a_2 (columns 0, 1, 2) become the ascending-i sums of w_i * (A_i a_c)
 * under the origin's binding and are then made orthonormal, with dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z and
 * unit(v) = v / sqrtf(dot(v, v)) per coordinate, which FAILS unless 0 < dot(v, v) < INFINITY:
 *   x = unit(a_0);   y = unit(a_1 - dot(x, a_1) * x);   z = unit((a_2 - dot(x, a_2) * x) - dot(y, a_2) * y)
 * When a unit fails the three old axes stay. Row 3 stays. An unbound pose stays bit for bit.
 *
 * SOLVE (pure host, fp64 in the written order, only + - * /, without contraction). Nodes are rigid: M_j = [R_j | t_j] with
 * R_j a rotation (the call does not test that). A CONSTRAINT c has src, dst, a time and a weight >= 0; it is bound by BIND
 * of src with its time (fp32) to the nodes i with weights wn_i, which are then widened; a constraint that is UNBOUND is
 * counted and otherwise ignored. A pin is a constraint with dst == src. With every float widened to double first and
 *   q_i = R_i (src - g_i), row r: (R[r][0]*d.x + R[r][1]*d.y) + R[r][2]*d.z;     phi_i.r = (q_i.r + g_i.r) + t_i.r
 *   res_c = (the ascending-i sum of wn_i * phi_i, from the first term) - dst
 *   res_jk = (((R_j (g_k - g_j)).r + g_j.r) + t_j.r - g_k.r) - t_k.r        for every k in EDGES(j), by (j, slot)
 *   energy = sum_c weight_c |res_c|^2 + w_reg sum_jk |res_jk|^2,   |v|^2 = (v.x*v.x + v.y*v.y) + v.z*v.z, each term added as
 *   energy + wgt * |v|^2, constraints first in index order, then the edges.
 * The unknown per node is (w, u), six numbers; the update is R_j <- Cayley(w) R_j with the Cayley map of sf_align.h and
 * t_j <- t_j + u. One Gauss-Newton ITERATION: with K(q) = -[q]x = (0, q.z, -q.y; -q.z, 0, q.x; q.y, -q.x, 0) the Jacobian
 * row r of a constraint has, in the six columns of node i, wn_i * K(q_i)[r][0..2] and wn_i * (r == k ? 1 : 0); that of an
 * edge has K(q)[r][.] and the unit row for node j, zeros and minus the unit row for node k. Residual by residual in the order
 * of the energy, row by row, the dense 6G x 6G system gets H[a][c] += wgt * (J[a] * J[c]) and b[a] += wgt * (J[a] * res.r)
 * over all listed columns a, c (the structural zeros included). `damping` is added to the diagonal. (H + damping I) x = -b
 * is solved by LDL^T without pivoting; a pivot that is not > 1e-9 * (bound constraints + edges) -- the test of the alignment
 * step, generalised to 6G dimensions -- is REFUSED: the solve stops with SFD_DEGENERATE and M is what it was before that
 * iteration. The transforms are kept in double across the iterations and rounded to float once, at the end.
 * The report holds energy[k], the energy before iteration k for k < iterations_done, and energy[iterations_done], the
 * energy of the transforms returned; the rest is 0.
 *
 * AFTER sfd_apply_maps the rule AFTER A CALL THAT CHANGES A MAP of sf_map_window.h holds for every map of the call: surfel
 * indices count as moved (the index image no longer describes where the surfels are), sf_map_get_index_map returns
 * SF_ERR_STATE until the next fuse with tick > 1; prediction, fuse, download and rebind work at once; count, tick, pose and
 * the statistics of the last fuse are unchanged.
 *
 * All functions return SF_OK or the SF_ERR_* codes of sf.h; sf_last_error() has the text. The calls that take maps are ordered
 * on the handle's HIP stream like a fuse and return after their results have been read back. One launch serves the whole
 * batch. The search for the nearest nodes is brute force: exact, no reach parameter, G distance tests per surfel.
 *
 * REFUSALS (SF_ERR_ARG unless said otherwise; nothing launched, nothing changed, outputs untouched): a null argument (M of
 * sfd_graph_set may be NULL: identities); n < 0 or n > 65535 (n == 0 is SF_OK); a map or a graph of another handle; the same
 * map twice in one call (a graph may serve several maps); a graph with G == 0 (SF_ERR_STATE); a time_window that is NaN or
 * negative; G outside 0 .. max_nodes in sfd_graph_set, outside 1 .. SFD_MAX_NODES in the
 * pure-host calls, above SFD_SOLVE_MAX_NODES in sfd_solve; a NaN or inf in M, in a pose handed to sfd_deform_poses, in a
 * constraint, or in the solve parameters (time_window may be +inf); a negative weight, w_reg or damping; iterations outside
 * 1 .. 32; a handle that has been destroyed, or a map or a graph whose handle was (SF_ERR_STATE); memory that cannot be grown
 * (the allocation's own code). Node positions and times may hold any value: a node with a NaN in them is never eligible.
 *
 * OUT OF SCOPE: node sampling in temporal order and the temporal pre-sort of the search; a sparse or device-side
 * factorisation, and more than SFD_SOLVE_MAX_NODES nodes in the solver (the dense system is 19 MB there); affine nodes in
 * the solver (apply takes any A); building constraints; writing anything back into a stream or a keyframe database (the
 * caller does that with sfd_deform_poses).
 */
#ifndef SF_DEFORM_H_
#define SF_DEFORM_H_

#include "sf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SFD_MAX_NODES 1024
#define SFD_SOLVE_MAX_NODES 256
#define SFD_MAX_ITERATIONS 32
#define SFD_OK 0
#define SFD_DEGENERATE 2

typedef struct sfd_graph sfd_graph;

typedef struct sfd_params {
    float   time_window; /* >= 0, +inf allowed, not NaN: a node is eligible when its time lies this close to the surfel's */
    int32_t reserved[7]; /* not read                                                                                      */
} sfd_params;            /* 32 bytes; sfd_params_bytes() reports it */

typedef struct sfd_counts {
    int32_t n_surfels;   /* the map's count                     */
    int32_t n_bound;     /* deformed                            */
    int32_t n_unbound;   /* left bit for bit                    */
    int32_t n_short;     /* of the bound, to fewer than 4 nodes */
    int32_t reserved[4]; /* 0                                   */
} sfd_counts;            /* 32 bytes; sfd_counts_bytes() reports it */

typedef struct sfd_info {
    int32_t max_nodes;
    int32_t n_nodes;     /* G of the last sfd_graph_set; 0 after sfd_graph_create */
    int32_t reserved[2]; /* 0 */
} sfd_info;              /* 16 bytes; sfd_info_bytes() reports it */

typedef struct sfd_constraint {
    float src[3];
    float dst[3];
    float time;          /* the tau src is bound with */
    float weight;        /* >= 0 */
} sfd_constraint;        /* 32 bytes; sfd_constraint_bytes() reports it */

typedef struct sfd_solve_params {
    float   time_window; /* as in sfd_params; it selects the nodes of a constraint and the edges */
    float   w_reg;       /* >= 0: the weight of the edge terms                                   */
    float   damping;     /* >= 0: added to the diagonal of the normal equations                  */
    int32_t iterations;  /* 1 .. 32                                                              */
    int32_t reserved[4]; /* not read                                                             */
} sfd_solve_params;      /* 32 bytes; sfd_solve_params_bytes() reports it */

typedef struct sfd_report {
    int32_t status;          /* SFD_OK or SFD_DEGENERATE                       */
    int32_t iterations_done;
    int32_t n_bound;         /* constraints bound to at least one node         */
    int32_t n_unbound;
    double  energy[33];      /* SOLVE above                                    */
} sfd_report;                /* 280 bytes; sfd_report_bytes() reports it */

int sfd_version(void); /* 1 */
size_t sfd_params_bytes(void);       /* 32 */
size_t sfd_counts_bytes(void);       /* 32 */
size_t sfd_info_bytes(void);         /* 16 */
size_t sfd_constraint_bytes(void);   /* 32 */
size_t sfd_solve_params_bytes(void); /* 32 */
size_t sfd_report_bytes(void);       /* 280 */

/* time_window +inf. These are parameter defaults, NOT tuned values. */
int sfd_default_params(sfd_params *p);
/* time_window +inf, w_reg 1, damping 1e-6, iterations 8. These are parameter defaults, NOT tuned values. */
int sfd_default_solve_params(sfd_solve_params *p);

/* Pure host, no handle, no GPU: SF_OK, or SF_ERR_ARG for null parameters or ones the refusal list names. */
int sfd_check_params(const sfd_params *p);
int sfd_check_solve_params(const sfd_solve_params *p);

/* A graph of at most max_nodes nodes (1 .. SFD_MAX_NODES) on h, with no nodes yet. It owns its device memory and the host
 * copy of its nodes; sf_destroy of h releases the memory and leaves a shell that every call answers with SF_ERR_STATE and
 * sfd_graph_destroy frees. */
int sfd_graph_create(sf_handle *h, int max_nodes, sfd_graph **out);
void sfd_graph_destroy(sfd_graph *graph);
int sfd_graph_info(const sfd_graph *graph, sfd_info *info);
/* The G nodes of the graph: pos 3 floats per node, times one, M 12 (NULL: identities). G == 0 empties it. */
int sfd_graph_set(sfd_graph *graph, int G, const float *pos, const float *times, const float *M);
/* What sfd_graph_set was given, for the graph's n_nodes nodes; any output may be NULL. */
int sfd_graph_get(const sfd_graph *graph, float *pos, float *times, float *M);

/* Node candidates from a map: the most confident surfel of every voxel of edge `spacing`, in surfel order -- what the
 * thinning of sf_join.h keeps at that cell, surfels outside its grid included --, positions to pos_out (3 floats each) and
 * init times to times_out, *count_out their number. More than max_nodes: SF_ERR_STATE, *count_out is the number, nothing
 * else is written. The map is unchanged. */
int sfd_sample_nodes(sf_map *map, float spacing, int max_nodes, float *pos_out, float *times_out, int *count_out);

/* Pure host, no handle, no GPU; the device compiles the same text. BIND of p with tau: returns m (0: UNBOUND) or SF_ERR_ARG. */
int sfd_bind_point(int G, const float *pos, const float *times, float time_window, const float p[3], float tau, int32_t idx_out[4], float w_out[4]);
/* DEFORM of s: returns m and writes out (which may be s); m == 0: out is s bit for bit. */
int sfd_deform_surfel(int G, const float *pos, const float *times, const float *M, float time_window, const float s[12], float out[12]);
/* EDGES of every node: 4 indices per node. */
int sfd_edges(int G, const float *pos, const float *times, float time_window, int32_t *edges_out);
/* POSE for n poses (16 floats each) with their taus; poses_out may be poses. */
int sfd_deform_poses(int G, const float *pos, const float *times, const float *M, float time_window, int n, const float *poses, const float *taus,
                     float *poses_out);

/* The binding of every surfel of maps[q] under graphs[q] to host memory: maps one after the other, 4 indices and 4 weights per
 * surfel (idx_out and w_out hold 4 * the sum of the counts). For diagnostics and tests; no map changes. */
int sfd_bind_maps(sf_handle *h, int n, sf_map *const *maps, sfd_graph *const *graphs, const sfd_params *params, int32_t *idx_out, float *w_out);

/* DEFORM of every surfel of maps[q] under graphs[q] with params[q], in place; counts_out[q] is filled. */
int sfd_apply_maps(sf_handle *h, int n, sf_map *const *maps, sfd_graph *const *graphs, const sfd_params *params, sfd_counts *counts_out);

/* SOLVE: M_inout (12 floats per node) holds the transforms to start from and receives the result; report_out is filled.
 * Returns SF_OK also when the report's status is SFD_DEGENERATE. */
int sfd_solve(int G, const float *pos, const float *times, int C, const sfd_constraint *constraints, const sfd_solve_params *solve_params, float *M_inout,
              sfd_report *report_out);

#ifdef __cplusplus
}
#endif
#endif
