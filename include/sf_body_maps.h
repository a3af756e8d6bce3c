/* sf_body_maps.h — body maps: every moving region fused into a surfel map of its own, carried along with its motion.
 *
 * A companion of sf.h, not part of its ABI: plain C declarations with the prefix sfp_, exported by libsf_hip.so (and its
 * precise and reference-order builds) only. The CPU oracle does not implement them and SF_ABI_VERSION does not count them;
 * sfp_version() versions this interface.
 *
 * sf_regions.h says what moved, sf_tracks.h whether it is the same thing as a frame ago, sf_bodies.h how it moved (the world
 * motion of its record), and the static room is a surfel map. The moving thing itself has no map: the static fusion gives
 * its pixels confidence 0. These calls keep them. A BODY MAP is an ordinary sf_map made with sf_map_create; it holds surfels
 * in the layout of sf.h, in world coordinates at the time of its last fuse. A fuse moves the whole map by the body's world
 * motion since then and folds the region's pixels of the new frame into it on a voxel grid: a pixel whose voxel holds a
 * surfel is averaged into it, a pixel whose voxel is empty starts a surfel. Views, scores, alignment, join and thin, the
 * window calls, download and PLY take the result like any other map.
 *
 * DEFINITIONS. s[0..11] is a surfel in the layout of sf.h (position + confidence; colour, weight, init time, last time;
 * normal + radius). Images are column-major like every image of sf.h: element (v, u) at v + u * rows, its PIXEL INDEX. All
 * arithmetic is fp32, one rounding per operation in the written order, without contraction; a comparison with a NaN operand
 * is false.
 *   pdot(a, b)   = (a.x * b.x + a.y * b.y) + a.z * b.z
 *   pcross(a, b) = (a.y * b.z - b.y * a.z,  a.z * b.x - b.z * a.x,  a.x * b.y - b.x * a.y)
 *   row(M, r, p) = ((M[r] * p.x + M[4 + r] * p.y) + M[8 + r] * p.z)      M a column-major 4 x 4; for a POSITION + M[12 + r]
 *                  is added last, for a NORMAL it is not
 *   min(x, y)    = y when y < x holds, else x
 *
 * ENTRY q of a call: a frame of rows x cols -- depth Z (float32), label image L (int32), optionally a colour image (uint8 x 3,
 * row-major, byte k of pixel (v, u) at (v * cols + u) * 3 + k, as the colour frames of sf.h; NULL stands for 128, 128, 128
 * everywhere) --, a camera C, a region label t >= 1, a map m, a motion W[q] (4 x 4, column-major, from world at the map's
 * time to world now; a NULL array W stands for identities, and the same arithmetic runs) and params. Several entries may share
 * one frame, with different labels and maps.
 *
 * BACK-PROJECTION under C:  P(v, u, z) = ((((float)u - cx) * z) / fx,  (((float)v - cy) * z) / fy,  z)
 *
 * PIXEL SURFEL of (v, u), z = Z(v, u):
 *  1 valid(x) = x > 0 && x <= z_max. The pixel HAS A NORMAL when 1 <= v <= rows - 2 and 1 <= u <= cols - 2, z and the four
 *    neighbour depths are valid, fabsf(Zn - z) <= normal_dz for each of the four neighbour depths Zn, and, with
 *      a = P(v, u + 1, Z(v, u + 1)) - P(v, u - 1, Z(v, u - 1))      b = P(v + 1, u, Z(v + 1, u)) - P(v - 1, u, Z(v - 1, u))
 *      c = pcross(a, b)      cc = pdot(c, c)
 *    cc > 0 && cc < INFINITY holds; then n = (c.x / s, c.y / s, c.z / s) with s = sqrtf(cc). The sign of n stays as computed:
 *    it points away from the camera, the convention of the map fusion. A pixel without a normal has no pixel surfel.
 *  2 P = P(v, u, z).
 *  3 radius:  r0 = (z / ((fx + fy) / 2.0f)) * 1.41421356237f;   radius = min(2.0f * r0, r0 / fabsf(n.z))
 *  4 X_r = row(C.pose, r, P) as a position, N_r = row(C.pose, r, n) as a normal, r = 0, 1, 2.
 *  5 colour: a channel value x in [0, 1] is the byte q = floorf(x * 255.0f + 0.5f) when 0 <= q <= 255 holds and the byte 0
 *    otherwise; for x >= 0 that is the rounding of the map fusion. The pixel's bytes B_k give x_k = (float)B_k / 255.0f, and
 *    colour = (float)((byte(x_0) << 16) + (byte(x_1) << 8) + byte(x_2)), which is (B_0 << 16) + (B_1 << 8) + B_2.
 *    Decoding a colour value c: k = (int)c when c >= 0 && c < 16777216 holds and 0 otherwise; channels
 *    (float)((k >> 16) & 255) / 255.0f, (float)((k >> 8) & 255) / 255.0f, (float)(k & 255) / 255.0f.
 *  6 the surfel is (X, conf_new | colour, 1, time, time | N, radius).
 *
 * VOXEL KEY of a position for `cell`, RANK of a confidence, and the TABLE (slots, hash, linear probing) are those of the
 * join header (sf_join.h), word for word:
 *   inv = 1.0f / cell, evaluated once on the host;  q_i = floorf(p_i * inv);  p is OUTSIDE THE GRID when any p_i or q_i is not
 *   finite or |q_i| >= 2^20; otherwise key = (uint64)(q_x + 2^20) << 42 | (uint64)(q_y + 2^20) << 21 | (uint64)(q_z + 2^20).
 *   rank(c), u the bits of c: NaN -> 0; sign set -> ~u; otherwise u | 0x80000000.
 *   A table for E elements has slots = the smallest power of two >= max(2 * E, 64), L = log2(slots); the first slot of a key
 *   is (key * 0x9E3779B97F4A7C15ull) >> (64 - L); probing is linear, (slot + 1) & (slots - 1).
 * The table of an entry is made for E = count + max(rows - 2, 0) * max(cols - 2, 0): the map's surfels and every pixel that
 * can have a normal. (The size is stated because a test has to be able to build keys that collide.)
 *
 * A FUSE does, per entry, with time = (float)tick of the map:
 *  MOVE.  Every surfel of the map: position s'[r] = row(W, r, s[0..2]) as a position, normal s'[8 + r] = row(W, r, s[8..10]) as a
 *    normal; everything else stays bit for bit.
 *  TABLE.  The moved surfels inside the grid fill the table. The REPRESENTATIVE of a voxel is its surfel of highest rank, among
 *    equal ranks the one of lowest index. Surfels outside the grid are moved and otherwise left alone.
 *  CANDIDATES.  A candidate is a pixel with L == t that has a pixel surfel whose X lies inside the grid. Every voxel that
 *    candidates touch has one WINNER: the candidate of lowest pixel index. (The reference fusion decides the same way, with an
 *    atomic minimum over candidates.) For the winner of a voxel:
 *      - the voxel holds a representative s: when pdot(N_s', N) >= min_dot holds (N_s' the moved normal of s), the winner is
 *        MERGED into s; otherwise it is counted in n_conflict and changes nothing;
 *      - the voxel holds no map surfel: the winner is ADDED: its pixel surfel is appended behind the map's own surfels, the
 *        added ones in ascending pixel index.
 *    Candidates that are not winners change nothing.
 *  MERGE of pixel surfel p into the moved representative s':
 *      w = fminf(s[5], max_weight)      den = w + 1.0f
 *      position, normal, radius and each of the three decoded colour channels become ((w * old) + new) / den, old the value of
 *      s' and new that of p; the colour is encoded again as in 5;
 *      the blended normal n is divided by sqrtf(nn), nn = pdot(n, n), when nn > 0 && nn < INFINITY holds; otherwise the normal
 *      of s' stays;
 *      s[3] = c + gain * (1.0f - c), c the old s[3];   s[5] = s[5] + 1.0f;   s[7] = time;   s[6] stays.
 *    A merged surfel may leave its voxel; the table is not rebuilt within a call.
 *  STATE.  After a successful call the map's tick is tick + 1, its pose is C.pose, its count the new count; the statistics of
 *    the last fuse are unchanged; and the rule AFTER A CALL THAT CHANGES A MAP of sf_map_window.h holds: surfel indices count as
 *    moved, sf_map_get_index_map returns SF_ERR_STATE until the next fuse with tick > 1; prediction, fuse, download and rebind
 *    work at once.
 *
 * sfp_move_maps does the MOVE alone, in place: count, tick, pose and statistics stay; the index-map rule above holds as well,
 * because the index image no longer describes where the surfels are.
 *
 * COUNTS. One sfp_counts per entry: n_pixels, the pixels with L == t; n_candidates; n_voxels, the occupied voxels of the moved
 * map; n_merged; n_added; n_conflict; n_out = count + n_added, the new count; one reserved word, written as 0.
 *
 * CAPACITY. When count + n_added exceeds the map's capacity in ANY entry the call returns SF_ERR_STATE, NO map of the call
 * changes -- not even by the move -- and counts_out is filled with what would have happened. For that the deciding passes
 * compute moved positions on the fly; the passes that change a map (move and merge in place, one lane per surfel; the ordered
 * append) run only after the counts have been read back. Both fuse calls therefore return after that read-back: a map's
 * count lives on the host.
 *
 * All functions return SF_OK or the SF_ERR_* codes of sf.h; sf_last_error() has the text. The calls that take maps are ordered
 * on the handle's HIP stream like a fuse. One set of launches serves the whole batch. A call needs 20 bytes of handle scratch
 * per slot, 4 per surfel and about 4.2 per pixel of every entry (the host form: 11 more per pixel for the frames); it
 * grows with the largest call and is freed with the handle.
 *
 * REFUSALS (SF_ERR_ARG unless said otherwise; nothing launched, nothing changed, counts_out untouched): a null argument
 * (the colour array, W, and single entries of the colour array may be NULL); n < 0 or n > 65535 (n == 0 is SF_OK); rows or
 * cols outside 1..4096 or rows * cols > 2^24; a region label < 1; a map of another handle; the same map twice in one call; a
 * non-finite camera or W entry, or fx or fy equal to 0; bad params: a NaN or inf, a cell that is not > 0 or whose 1.0f / cell
 * is not finite, z_max or normal_dz outside (0, 32], min_dot outside [-1, 1], conf_new outside [0, 1], gain outside (0, 1],
 * max_weight < 1; a handle that has been destroyed, or a map whose handle was (SF_ERR_STATE); scratch that cannot be grown (the
 * allocation's own code). A probe walk that visits every slot without finding its key or an empty slot makes the call return
 * SF_ERR_STATE with no map changed; at a load of one half that cannot happen, and every loop is bounded so that it cannot
 * hang either.
 *
 * OUT OF SCOPE: searching neighbouring voxels (a surface point near a voxel face can start a second surfel next door, so the
 * count grows for some frames after the surface has been covered); removing surfels (sfw_cull_maps by age works, because the
 * tick advances); free-space violations; photometric terms; a tracker-owned table of maps; checkpointing; writing anything
 * back into a stream.
 */
#ifndef SF_BODY_MAPS_H_
#define SF_BODY_MAPS_H_

#include "sf_bodies.h"
#include "sf_join.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The camera of sf_tracks.h under a name of this interface: the same fields at the same offsets, so that a record of either
 * header can be handed to the other as it is. (Every companion header keeps its prefix to itself; the library asserts that
 * the layouts agree.) */
typedef struct sfp_camera {
    float pose[16];        /* camera-to-world, column-major */
    float cx, cy, fx, fy;  /* pixels; fx, fy != 0 */
} sfp_camera;              /* 80 bytes; sfp_camera_bytes() reports it */

typedef struct sfp_params {
    float   cell;        /* edge of a voxel in metres: finite, > 0, and 1.0f / cell finite */
    float   z_max;       /* metres, 0 < . <= 32: depths beyond it are not used */
    float   normal_dz;   /* metres, 0 < . <= 32: the largest depth step to a neighbour a normal is taken across */
    float   min_dot;     /* -1 <= . <= 1: a pixel is merged into a surfel whose normal it meets at least this well */
    float   conf_new;    /* 0 <= . <= 1: the confidence of an added surfel */
    float   gain;        /* 0 < . <= 1: a merge closes this share of the gap between the confidence and 1 */
    float   max_weight;  /* >= 1: the weight a surfel's history has at most against one new pixel */
    int32_t reserved;    /* not read */
} sfp_params;            /* 32 bytes; sfp_params_bytes() reports it */

typedef struct sfp_counts {
    int32_t n_pixels;     /* pixels with L == t */
    int32_t n_candidates; /* of those, with a pixel surfel inside the grid */
    int32_t n_voxels;     /* occupied voxels of the moved map */
    int32_t n_merged;     /* winners merged into a representative */
    int32_t n_added;      /* winners appended */
    int32_t n_conflict;   /* winners that failed the normal gate */
    int32_t n_out;        /* count + n_added */
    int32_t reserved;     /* 0 */
} sfp_counts;             /* 32 bytes; sfp_counts_bytes() reports it */

int sfp_version(void); /* 1 */
size_t sfp_params_bytes(void); /* 32 */
size_t sfp_counts_bytes(void); /* 32 */
size_t sfp_camera_bytes(void); /* 80 */

/* cell 0.01, z_max 8, normal_dz 0.05, min_dot 0.8, conf_new 0.1, gain 0.25, max_weight 32. These are parameter defaults, NOT
 * tuned values: nobody has tuned them on real data. */
int sfp_default_params(sfp_params *p);

/* Pure host, no handle, no GPU: SF_OK, or SF_ERR_ARG for null parameters or ones the refusal list names. */
int sfp_check_params(const sfp_params *p);

/* Pure host, no handle, no GPU: PIXEL SURFEL of the pixel (v, u), taken to be interior, from its depth and its neighbours':
 * depths[0..4] = Z(v, u), Z(v, u - 1), Z(v, u + 1), Z(v - 1, u), Z(v + 1, u) (any values, NaN and inf included); colour
 * three bytes or NULL for 128, 128, 128; time any float. Returns 1 and writes the 12 floats, or 0 for a pixel without a normal
 * (out untouched); SF_ERR_ARG for a null argument, a camera or params a fuse would refuse. The device compiles the same text. */
int sfp_pixel_surfel(const float depths[5], int v, int u, const sfp_camera *cam, const uint8_t *colour, const sfp_params *p, float time, float out[12]);

/* Pure host: MERGE of the pixel surfel `pixel` into the (moved) map surfel s with gain and max_weight of p; out may be s.
 * SF_ERR_ARG for a null argument or bad params. The device compiles the same text. */
int sfp_merge_surfel(const sfp_params *p, const float s[12], const float pixel[12], float time, float out[12]);

/* MOVE every surfel of maps[q] by W + 16 q, in place (W NULL: identities). The maps are distinct and belong to h. Asynchronous
 * on the handle's stream. */
int sfp_move_maps(sf_handle *h, int n, sf_map *const *maps, const float *W);

/* FUSE entry q < n: the pixels with labels[q] == region_labels[q] of the frame (depth[q], labels[q], colour[q]) seen by
 * cams[q] into maps[q], moved by W + 16 q first, under params[q]; counts_out[q] is filled. depth and labels are arrays of n
 * HOST pointers to rows x cols images; colour is NULL or such an array, whose entries may be NULL. */
int sfp_fuse_images(sf_handle *h, int rows, int cols, int n, const float *const *depth, const int32_t *const *labels, const uint8_t *const *colour,
                    const sfp_camera *cams, const int32_t *region_labels, sf_map *const *maps, const float *W, const sfp_params *params,
                    sfp_counts *counts_out);

/* The same with DEVICE pointers in the (host) arrays depth, labels and colour -- the label images are what
 * sfr_label_images_device wrote, the depths and colours the caller's buffers, 4-byte aligned --; cams, region_labels, maps, W,
 * params and counts_out are host memory as above. */
int sfp_fuse_images_device(sf_handle *h, int rows, int cols, int n, const void *const *depth, const void *const *labels, const void *const *colour,
                           const sfp_camera *cams, const int32_t *region_labels, sf_map *const *maps, const float *W, const sfp_params *params,
                           sfp_counts *counts_out);

#ifdef __cplusplus
}
#endif
#endif
