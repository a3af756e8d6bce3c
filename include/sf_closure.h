/* sf_closure.h — loop-closure constraints from two sightings of a place, built on the device.
 *
 * A companion of sf.h, not part of its ABI: plain C declarations with the prefix sfc_, exported by libsf_hip.so (and its
 * precise and reference-order builds) only. The CPU oracle does not implement them and SF_ABI_VERSION does not count them;
 * sfc_version() versions this interface.
 *
 * The relocalisation chain runs from a proposed pose (sf_keyframes.h) over its score (sf_score.h) and its refinement
 * (sf_align.h) to the solve and the bend of sf_deform.h, whose solve takes an array of point constraints and names "building
 * constraints" as out of its scope. This interface builds them, as ElasticFusion (Whelan et al., RSS 2015) does: the ACTIVE
 * part of the model (what the stream saw lately, under the pose it believes) and the INACTIVE part (what it saw long ago) are
 * drawn from the same camera; where both are drawn, the active point is sent from the drifted pose to the refined one, and
 * the inactive point is pinned. Many closures per call; only the records come back, no images.
 *
 * DEFINITIONS. s[0..11] is a surfel in the layout of sf.h. All arithmetic is fp32, one rounding per operation in the written
 * order, without contraction; a comparison with a NaN operand is false.
 *
 * ENTRY q has four parts: a map map_new and a map map_old -- both only read; they may be the same map, and either may appear
 * in any number of entries --, a view view_from (the pose the stream believes it has; its max_age selects the active part of
 * map_new with that map's tick), a view view_to (the pose refined against the old part, as the refinement of sf_align.h
 * returns it) and parameters sfc_params. The two views must agree bit for bit in rows, cols, cx, cy, fx, fy; max_depth,
 * min_confidence and max_age belong to each view's own draw and may differ; shade is not read.
 * A caller gets the old part of one map with sfw_extract (a filter with max_age and invert = 1) and sfw_append into a second
 * map (sf_map_window.h).
 *
 * IMAGES. A is the drawing of map_new from view_from by GEOMETRY of sf_view.h: per pixel the winning surfel index a (-1 when
 * nothing is drawn) and zA, the float the depth image of a render holds. O is the same of map_old from view_to: o and zO.
 * The views share intrinsics, so a pixel of A and the same pixel of O are the same camera ray, seen under the believed pose
 * in A and under the refined pose in O.
 *
 * SAMPLES. With stride s in 1 .. 4096 and s2 = s / 2 (integer): sample columns are x = s2 + i*s < cols, sample rows are
 * y = s2 + j*s < rows; sample k counts y in the outer loop and x in the inner loop, both ascending. No sample is SF_OK, with
 * zero counts.
 *
 * PER SAMPLE, with sa, so the surfel records of a and o:
 *   both  = a >= 0 && o >= 0
 *   dz    = fabsf(zA - zO)
 *   near  = both && dz <= gate_abs + gate_rel * zO          (gate_abs may be +inf: ElasticFusion's rule, overlap alone)
 *   apart = near && sa[6] - so[6] > min_time_gap            (min_time_gap is finite or -inf; choose at least twice the
 *           time_window of the solve, so that a source and its pin cannot share a node)
 *   LINK, made when apart:
 *     src = sa[0..2] as stored: the position the bend of sf_deform.h will bind
 *     h = inverse(view_from.pose) * src, exactly as the drawing computes the camera position (the same pose inversion, and
 *         h.r = T[r]*src.x + T[4+r]*src.y + T[8+r]*src.z + T[12+r], left to right)
 *     dst.r = ((P[r]*h.x + P[4+r]*h.y) + P[8+r]*h.z) + P[12+r]   with P = view_to.pose
 *     time = sa[6], weight = w_link
 *   PIN: src = dst = so[0..2], time = so[6], weight = w_pin; made when a LINK is made (pins == 1), when o >= 0 (pins == 2),
 *     never (pins == 0)
 *   A record is DROPPED when its src, dst or time holds a value that is not finite: it is not written and is counted. A LINK
 *   that drops does not take its pin (pins == 1) with it.
 * OUTPUT ORDER is sample order; at one sample the LINK comes before the PIN.
 *
 * COUNTS, one sfc_counts per entry: n_samples, n_new (a >= 0), n_old (o >= 0), n_both, n_near, n_apart, n_links and n_pins
 * (written), n_dropped, first (the index of the entry's first record in the call's output), and
 *   sum_dz    = the sum over near of (int64)rintf(fminf(dz, 32.f) * 16384.f)
 *   sum_shift = the same quantisation of sqrtf((dx*dx + dy*dy) + dz*dz) of dst - src, over the links written.
 * The sums are integers: no result depends on an order of arrival.
 *
 * A RECORD (sfc_record) is the point constraint of sf_deform.h field for field -- src, dst, time, weight, 32 bytes --, so
 * the output array is handed to that header's solve as its constraint array as it is.
 *
 * A BUILD only reads its maps: afterwards the maps, sf_map_info, sf_map_get_index_map and the prediction are what they were.
 * It is ordered on the handle's HIP stream and returns after the read-back. The counting pass comes first; the writing pass
 * runs only after the counts are back and the capacity is checked (the order of sf_body_maps.h).
 *
 * All functions return SF_OK or the SF_ERR_* codes of sf.h; sf_last_error() has the text.
 *
 * REFUSALS (SF_ERR_ARG unless said otherwise; nothing launched, outputs untouched): a null argument; n < 0 or 2n > 65535
 * (n == 0 is SF_OK); a map or a builder of another handle; a view that sfv_check_view refuses; two views of an entry that
 * differ in size or intrinsics; stride outside 1 .. 4096; pins outside 0 .. 2; a NaN in the params; a negative gate or weight;
 * gate_rel or a weight that is inf; min_time_gap that is +inf; max_records < 0, or out == NULL with max_records > 0; a
 * destroyed handle, or a map or a builder whose handle was destroyed (SF_ERR_STATE); memory that cannot be grown (the
 * allocation's own code).
 * More records than max_records is SF_ERR_ARG too, but found after the counting pass: counts_out is filled, out is untouched.
 *
 * OUT OF SCOPE: a device-pointer form of the output; a device-side split of a map into two; constraints from a live frame
 * instead of the drawn active part; relative constraints between earlier closures; choosing the time window of the solve or
 * the gates.
 */
#ifndef SF_CLOSURE_H_
#define SF_CLOSURE_H_

#include "sf.h"
#include "sf_view.h"
#include "sf_deform.h"

#ifdef __cplusplus
extern "C" {
#endif

/* what sfc_link_sample found: the bits of its return value */
#define SFC_FOUND_BOTH 1
#define SFC_FOUND_NEAR 2
#define SFC_FOUND_APART 4
#define SFC_FOUND_LINK 8          /* a LINK was written             */
#define SFC_FOUND_PIN 16          /* a PIN was written              */
#define SFC_FOUND_LINK_DROPPED 32 /* a LINK was made and dropped    */
#define SFC_FOUND_PIN_DROPPED 64  /* a PIN was made and dropped     */
#define SFC_MAX_STRIDE 4096

typedef struct sfc_builder sfc_builder;

typedef struct sfc_params {
    int32_t stride;       /* 1 .. 4096: every stride-th pixel of every stride-th row, from stride / 2        */
    int32_t pins;         /* 0: no pins; 1: a pin with every link; 2: a pin wherever the old part is drawn   */
    float   gate_abs;     /* >= 0, +inf allowed: metres of |zA - zO| that still count as the same surface    */
    float   gate_rel;     /* >= 0, finite: ... plus this fraction of zO                                      */
    float   min_time_gap; /* finite or -inf: a link needs sa[6] - so[6] > min_time_gap                       */
    float   w_link;       /* >= 0, finite: the weight of a LINK                                              */
    float   w_pin;        /* >= 0, finite: the weight of a PIN                                               */
    int32_t reserved;     /* not read                                                                        */
} sfc_params;             /* 32 bytes; sfc_params_bytes() reports it */

typedef struct sfc_counts {
    int32_t n_samples;
    int32_t n_new;        /* a >= 0                                   */
    int32_t n_old;        /* o >= 0                                   */
    int32_t n_both;
    int32_t n_near;
    int32_t n_apart;
    int32_t n_links;      /* written                                  */
    int32_t n_pins;       /* written                                  */
    int32_t n_dropped;    /* records made and not written             */
    int32_t first;        /* the entry's first record in the output   */
    int32_t reserved[2];  /* 0                                        */
    int64_t sum_dz;       /* COUNTS above                             */
    int64_t sum_shift;
} sfc_counts;             /* 64 bytes; sfc_counts_bytes() reports it */

typedef struct sfc_record {
    float src[3];
    float dst[3];
    float time;
    float weight;
} sfc_record;             /* 32 bytes: the point constraint of sf_deform.h, field for field */

int sfc_version(void); /* 1 */
size_t sfc_params_bytes(void); /* 32 */
size_t sfc_counts_bytes(void); /* 64 */

/* stride 4, pins 1, gate_abs 0.1, gate_rel 0.05, min_time_gap 0, w_link 1, w_pin 1. These are parameter defaults, NOT tuned values. */
int sfc_default_params(sfc_params *p);

/* Pure host, no handle, no GPU: SF_OK, or SF_ERR_ARG for null parameters or ones the refusal list names. */
int sfc_check_params(const sfc_params *p);

/* Pure host: 2 x the number of samples of `view` at `stride`, the bound a caller sizes the output of one entry by; SF_ERR_ARG
 * (negative) for a view sfv_check_view refuses or a stride outside 1 .. 4096. */
int sfc_max_records(const sfv_view *view, int stride);

/* Pure host; the device compiles the same text. PER SAMPLE for one sample: sa and so are the surfels a and o (12 floats each;
 * NULL: nothing drawn there), zA and zO their depths, pose_from and pose_to the poses of the two views (column-major, finite).
 * Writes the records made, the LINK before the PIN, to out (room for 2) and their number to *n_out; returns the SFC_FOUND_*
 * bits, or SF_ERR_ARG (negative). */
int sfc_link_sample(const float *sa, const float *so, float zA, float zO, const float pose_from[16], const float pose_to[16], const sfc_params *params,
                    sfc_record out[2], int32_t *n_out);

/* A builder on h. It owns the device memory its calls use; sf_destroy of h releases the memory and leaves a shell that every
 * call answers with SF_ERR_STATE and sfc_builder_destroy frees. */
int sfc_builder_create(sf_handle *h, sfc_builder **out);
void sfc_builder_destroy(sfc_builder *builder);

/* n entries in one set of launches: the records of all entries, one entry after the other, to HOST memory out (room for
 * max_records); counts_out[q] is always filled. More records than max_records: SF_ERR_ARG, the counts are filled and nothing
 * is written to out. out == NULL with max_records == 0 asks for the sizes only. */
int sfc_build(sfc_builder *builder, int n, sf_map *const *maps_new, sf_map *const *maps_old, const sfv_view *views_from, const sfv_view *views_to,
              const sfc_params *params, sfc_record *out, int max_records, sfc_counts *counts_out);

#ifdef __cplusplus
}
#endif
#endif
