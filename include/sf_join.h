/* sf_join.h — join and thin surfel maps on a voxel grid: merge, decimate.
 *
 * A companion of sf.h, not part of its ABI: plain C declarations with the prefix sfj_, exported by libsf_hip.so (and its
 * precise and reference-order builds) only. The CPU oracle does not implement them and SF_ABI_VERSION does not count them;
 * sfj_version() versions this interface.
 *
 * Two maps that saw the same room cannot be put together by appending one to the other: every surface both saw would be
 * stored twice, and the prediction would resolve the duplicates in buffer order. And a dense map can be made smaller only by
 * age, distance or confidence (sf_map_window.h), not by density. Both operations need one primitive, a spatial index over a
 * map's surfels. Here it is a voxel occupancy table in device memory, built with integer keys and device-scope atomics; its
 * results are a function of the inputs alone. On top of it:
 *   - sfj_thin_maps keeps one surfel per occupied voxel, the most confident one (sfj_thin_extract copies that set out and
 *     leaves the map alone: a tenth of a dense map for a viewer or an archive);
 *   - sfj_merge_maps appends to a destination the surfels of a source, moved into the destination's frame, whose voxel the
 *     destination does not occupy yet.
 *
 * DEFINITIONS. s[0..11] is a surfel in the layout of sf.h (position + confidence; colour, -, init time, last time; normal +
 * radius). All arithmetic is fp32, one rounding per operation written, without contraction.
 *
 * VOXEL KEY of a position p for a cell size `cell`:
 *   inv = 1.0f / cell                       evaluated once, on the host
 *   q_i = floorf(p_i * inv)                 i = x, y, z
 *   p is OUTSIDE THE GRID when any p_i or q_i is not finite or |q_i| >= 2^20; otherwise
 *   key = (uint64)(q_x + 2^20) << 42 | (uint64)(q_y + 2^20) << 21 | (uint64)(q_z + 2^20)
 * The top bit of a key is clear, so ~0ull is never a key: it marks an empty slot.
 *
 * RANK of a confidence c = s[3], u its bits: NaN -> 0; sign set -> ~u; otherwise -> u | 0x80000000. It orders like the
 * numbers; -0 ranks below +0 and a NaN below every number.
 *
 * TABLE for `count` surfels: slots = the smallest power of two >= max(2 * count, 64), L = log2(slots); the first slot of a key
 * is (key * 0x9E3779B97F4A7C15ull) >> (64 - L); probing is linear, (slot + 1) & (slots - 1). The load never exceeds one half.
 * (The hash is stated because a test has to be able to build keys that collide.)
 *
 * THIN. The map keeps, for every occupied voxel, one surfel: the one of highest rank, among equal ranks the one of lowest
 * index. Every surfel outside the grid is kept. What is kept is kept bit for bit and in its old order (the stable partition
 * of sf_map_window.h under this predicate). kept = n_voxels + n_outside.
 *
 * MERGE. T is 4 x 4, column-major, from the source's world frame to the destination's. A source surfel s is examined in this
 * order:
 *   1. with min_confidence > 0: unless s[3] >= min_confidence holds (a NaN fails) it is counted in n_below, and that is all;
 *   2. x' = ((T[0]*x + T[4]*y) + T[8]*z) + T[12],  y' = ((T[1]*x + T[5]*y) + T[9]*z) + T[13],
 *      z' = ((T[2]*x + T[6]*y) + T[10]*z) + T[14]; the normal goes through the upper 3 x 3 the same way, without the last term;
 *   3. p' outside the grid: counted in n_outside, and added;
 *   4. the voxel of p' holds a destination surfel: counted in n_shared, and not added;
 *   5. otherwise added.
 * The added surfels are appended behind the destination's own, in source order, with p', n' and the source's confidence,
 * colour and radius; with stamp >= 0, s[6] = s[7] = (float)stamp, otherwise the source's times. Destination surfels outside
 * the grid occupy nothing. The source is never changed, the destination's own surfels are not touched, source surfels are
 * not tested against each other. added = n_in - n_below - n_shared. When the destination's count + added exceeds its
 * capacity in ANY entry, the call returns SF_ERR_STATE, no map of the call changes, and counts_out is filled (n_out is what
 * would have been added).
 *
 * All functions return SF_OK or the SF_ERR_* codes of sf.h; sf_last_error() has the text. Those that take maps are ordered
 * on the handle's HIP stream like a fuse and return after the counts have been read back. One set of launches serves the
 * whole batch. A call needs 16 bytes of handle scratch per slot (merge: 8) and 4 per surfel; it grows with the largest call
 * and is freed with the handle.
 *
 * AFTER A CALL THAT CHANGES A MAP (sfj_thin_maps, sfj_merge_maps for its destinations, without dry_run) the rule of the same
 * name in sf_map_window.h holds unchanged: surfel indices have moved, sf_map_get_index_map returns SF_ERR_STATE until the
 * next fuse with tick > 1; prediction, fuse, download and rebind work at once; tick, pose and the statistics of the last fuse
 * are unchanged; count is the new count.
 *
 * REFUSALS (SF_ERR_ARG unless said otherwise; nothing launched, nothing changed, counts_out untouched): a null argument (T
 * may be null); n < 0 (n == 0 is SF_OK) or n > 65535; a map of another handle; the same map twice among the maps of a thin or
 * the destinations of a merge; a map that is a source in one entry and a destination in any entry (a source may appear in
 * several entries); bad params; a non-finite entry of T; a map whose handle was destroyed (SF_ERR_STATE); scratch that cannot be
 * grown (the allocation's own code). A probe walk that visits every slot without finding its key or an empty slot makes the
 * call return SF_ERR_STATE with no map changed; at a load of one half that cannot happen, and every loop is bounded so that
 * it cannot hang either.
 *
 * OUT OF SCOPE: averaging the attributes or accumulating the confidence of surfels that share a voxel; thinning the
 * destination during a merge; a grid with an origin or a rotation; hierarchical levels of detail; any reordering of
 * surfels; writing a refined pose into a stream.
 */
#ifndef SF_JOIN_H_
#define SF_JOIN_H_

#include "sf.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sfj_params {
    float   cell;           /* edge of a voxel in metres: finite, > 0, and 1.0f / cell finite                       */
    float   min_confidence; /* merge, enabled when > 0: source surfels with s[3] >= min_confidence only; not NaN   */
    int32_t stamp;          /* merge: >= 0 sets init and last time of the added surfels, < 0 keeps the source's    */
    int32_t dry_run;        /* 0, or 1: fill the counts and change nothing                                         */
    int32_t reserved[4];    /* pads the struct to 32 bytes; not read                                               */
} sfj_params;

typedef struct sfj_counts {
    int32_t n_in;        /* surfels examined: the map's (thin), the source's (merge)                                */
    int32_t n_outside;   /* of those, outside the grid (merge: after the confidence test and the transform)         */
    int32_t n_voxels;    /* distinct occupied voxels of the map that fills the table: the map (thin), the destination (merge) */
    int32_t n_below;     /* merge: failed the confidence test                                                       */
    int32_t n_shared;    /* merge: their voxel holds a destination surfel                                           */
    int32_t n_out;       /* kept (thin) or added (merge)                                                            */
    int32_t reserved[2]; /* 0                                                                                       */
} sfj_counts;

int sfj_version(void); /* 1 */
size_t sfj_params_bytes(void); /* sizeof(sfj_params) = 32 */
size_t sfj_counts_bytes(void); /* sizeof(sfj_counts) = 32 */

/* cell 0.02f, min_confidence 0, stamp -1, dry_run 0: parameter defaults, not tuned values. */
int sfj_default_params(sfj_params *p);

/* Pure host, no handle, no GPU: SF_OK, or SF_ERR_ARG for null params, a cell that is not finite or not > 0 or whose 1.0f / cell
 * is not finite, a NaN min_confidence, a dry_run that is neither 0 nor 1. */
int sfj_check_params(const sfj_params *p);

/* Pure host: the slots of a table for `count` surfels (TABLE above), count in 0 .. 2^29; SF_ERR_ARG otherwise. */
int sfj_table_slots(int count);

/* Pure host: 1 and *key for a position in the grid, 0 (and *key untouched) for one outside; SF_ERR_ARG for a null argument or
 * bad params. */
int sfj_voxel_key(const sfj_params *p, const float pos[3], uint64_t *key);

/* Pure host: the first slot of `key` in a table of `slots` slots (a power of two, 64 .. 2^30); SF_ERR_ARG otherwise. */
int sfj_hash_slot(uint64_t key, int slots);

/* THIN every maps[q] with params[q] (cell and dry_run are read); counts_out[q] is filled. The maps are distinct and belong to
 * h; params and counts_out hold n entries. */
int sfj_thin_maps(sf_handle *h, int n, sf_map *const *maps, const sfj_params *params, sfj_counts *counts_out);

/* The surfels a thin would keep, to host memory, in order; the map is unchanged, bit for bit. counts_out->n_out = their
 * number. More than max_count: SF_ERR_ARG and nothing is written to surfels_out. surfels_out may be NULL with max_count = 0
 * to ask for the size (SF_OK when nothing is kept). dry_run is not read. */
int sfj_thin_extract(sf_map *m, const sfj_params *p, float *surfels_out, int max_count, sfj_counts *counts_out);

/* MERGE src[q] into dst[q] with T + 16 q (T null: n identities; the same arithmetic runs) and params[q]; counts_out[q] is
 * filled. */
int sfj_merge_maps(sf_handle *h, int n, sf_map *const *dst, sf_map *const *src, const float *T, const sfj_params *params, sfj_counts *counts_out);

#ifdef __cplusplus
}
#endif
#endif
