/* sf_map_window.h — bounded surfel maps: count, cull, extract, page out and append.
 *
 * A companion of sf.h, not part of its ABI: plain C declarations with the prefix sfw_, exported by libsf_hip.so (and its
 * precise and reference-order builds) only. The CPU oracle does not implement them and SF_ABI_VERSION does not count them;
 * sfw_version() versions this interface.
 *
 * A sf_map only grows: the drivers run GlobalModel::clean with time_delta = INT_MAX, and a fuse that needs more than the
 * map's capacity truncates it (SF_ERR_STATE). With these calls a service keeps a map inside a budget, on the device and for
 * many maps per call:
 *   - drop what the camera has not seen for a while, or what is far from it (sfw_cull_maps);
 *   - move that part to host memory and bring it back later (sfw_page_out, sfw_append);
 *   - fetch only the stable surfels (sfw_extract with min_confidence).
 * All of them are one primitive: an order-preserving (stable) partition of the 48-byte surfel records by a per-surfel
 * predicate, from the map's buffer into its second buffer, which is idle between two fuses. The order matters: the
 * prediction resolves depth ties in buffer order and GlobalModel::clean is an ordered compaction.
 *
 * THE FILTER. s[0..11] is a surfel in the layout of sf.h (position + confidence; colour, -, init time, last time; normal +
 * radius). A surfel is SELECTED when every enabled test holds; `invert` selects the complement of that set. All arithmetic
 * is fp32 in the order written, without contraction. A comparison with a NaN operand is false: such a surfel is not
 * selected, or is selected under `invert`. With no test enabled every surfel is selected. A NaN in min_confidence, radius or
 * centre is SF_ERR_ARG.
 *
 * All functions return SF_OK or the SF_ERR_* codes of sf.h; sf_last_error() has the text. Those that take maps are ordered
 * on the handle's HIP stream like a fuse and return after the counts have been read back.
 *
 * AFTER A CALL THAT CHANGES A MAP (sfw_cull_maps, sfw_page_out, sfw_append) surfel indices have moved: the index image of
 * the last fuse no longer describes the map, and sf_map_get_index_map returns SF_ERR_STATE until the next fuse with
 * tick > 1 renders a new one. sf_map_predict*, sf_map_fuse*, sf_map_download and sfm_map_rebind work at once. Tick, pose and
 * the statistics of the last fuse (sf_map_info) are unchanged; count is the new count.
 *
 * REFUSALS (SF_ERR_ARG unless said otherwise; nothing launched, nothing changed): a null argument; n < 0 (n == 0 is SF_OK);
 * a map of another handle; the same map twice in a batch; a bad filter; a map whose handle was destroyed (SF_ERR_STATE, as in
 * sf_map_download).
 */
#ifndef SF_MAP_WINDOW_H_
#define SF_MAP_WINDOW_H_

#include "sf.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sfw_filter {
    float   min_confidence; /* test A, enabled when > 0:  s[3] >= min_confidence                                   */
    int32_t max_age;        /* test B, enabled when >= 0: (float)tick - s[7] <= (float)max_age   (tick: the map's) */
    float   centre[3];      /* test C, enabled when radius > 0, world frame:                                       */
    float   radius;         /*   dx = s[0]-centre[0], ...;  (dx*dx + dy*dy) + dz*dz <= radius*radius               */
    int32_t invert;         /* 0: selected = every enabled test holds; 1: the complement of that set               */
    int32_t reserved;       /* pads the struct to 32 bytes; not read                                               */
} sfw_filter;

int sfw_version(void); /* 1 */
size_t sfw_filter_bytes(void); /* sizeof(sfw_filter) = 32 */

/* Pure host, no handle, no GPU: SF_OK, or SF_ERR_ARG for a null filter or a NaN in min_confidence, radius or centre. */
int sfw_check_filter(const sfw_filter *f);

/* selected[q] = how many surfels of maps[q] filters[q] selects. Nothing changes. */
int sfw_count_maps(sf_handle *h, int n, sf_map *const *maps, const sfw_filter *filters, int *selected);

/* Afterwards maps[q] holds exactly the surfels filters[q] selects, in their old order; count = kept[q]. One set of launches
 * for the whole batch. The maps are distinct and belong to h; filters holds n entries. */
int sfw_cull_maps(sf_handle *h, int n, sf_map *const *maps, const sfw_filter *filters, int *kept);

/* The selected surfels to host memory, in order; the map is unchanged, bit for bit. *count = the number selected. More than
 * max_count: SF_ERR_ARG and nothing is written to surfels_out. surfels_out may be NULL with max_count = 0 to ask for the
 * size (SF_OK when nothing is selected). */
int sfw_extract(sf_map *m, const sfw_filter *f, float *surfels_out, int max_count, int *count);

/* The surfels NOT selected move to host memory, in order, and leave the map; the selected ones stay, in order. *count = the
 * number moved out. More than max_count: SF_ERR_ARG, *count is the number needed, neither the map nor surfels_out changes. */
int sfw_page_out(sf_map *m, const sfw_filter *f, float *surfels_out, int max_count, int *count);

/* Page in: `count` surfels are appended behind the map's own. count + the map's count > capacity: SF_ERR_STATE and nothing
 * changes. */
int sfw_append(sf_map *m, const float *surfels, int count);

#ifdef __cplusplus
}
#endif
#endif
