/* sf_regions.h — moving regions: connected components of the dynamic pixels of many frames per call, with statistics.
 *
 * A companion of sf.h, not part of its ABI: plain C declarations with the prefix sfr_, exported by libsf_hip.so (and its
 * precise and reference-order builds) only. The CPU oracle does not implement them and SF_ABI_VERSION does not count them;
 * sfr_version() versions this interface.
 *
 * The solver gives every pixel a static weight b. These calls answer what moved, where, and how large it was, on the
 * device, for many frames per call: a label image and one integer record per region. A call only READS its streams:
 * afterwards the streams, maps, predictions and the view / score / keyframe scratch are what they were.
 *
 * IMAGES are column-major float32 like every image of sf.h: element (v, u) at v + u * rows. zf is depth, bf the static
 * weight (the image sf_get_b_image returns). All float arithmetic is fp32 in the written order without contraction; a
 * comparison with a NaN operand is false.
 *
 * MASK.  M(p) = zf > 0 && zf <= z_max && (use_b ? bf < b_max : true).
 * NaN depth, +inf depth, NaN b and b == b_max are all outside the mask. With use_b = 0 the call segments a depth image into
 * depth-continuous pieces and the b pointer is not read.
 *
 * LINK.  Two neighbouring pixels p, q, both in M, are linked when
 *   fabsf(zp - zq) <= dz_abs + dz_rel * fminf(zp, zq).
 * The test is symmetric and every operand is finite because of z_max. With connectivity 4 the neighbours are (v +- 1, u)
 * and (v, u +- 1); connectivity 8 adds the four diagonals. A COMPONENT is a class of the transitive closure of the links: a
 * ramp of small steps is one component however far apart its ends are, and a person in front of a moving door is two.
 *
 * NUMBERING.  The `first` of a component is its smallest index v + u * rows. A component with n >= min_pixels is a REGION.
 * Regions are numbered 1 .. R in ascending first.
 *
 * LABEL IMAGE (int32, column-major, optional): 0 outside M; -1 in M but in a component smaller than min_pixels; k in region
 * k. The label image always carries all R numbers, even when max_regions is smaller.
 *
 * REGION RECORD.  The depth quantum is zq = (int32)rintf(zf * 1024.f), at most 32768. z_min, z_max and sum_z are over zq;
 * sum_b is the sum of (int32)rintf(fminf(fmaxf(bf, 0.f), 1.f) * 4096.f) when use_b is set, else 0. Centroid and mean depth
 * are sum_v / n, sum_u / n and sum_z / 1024 / n; the caller back-projects with its own intrinsics. Everything is an integer,
 * so a record depends neither on the order of summation nor on the batch it was computed in.
 * Region records n_written .. max_regions - 1 of an entry are written as zeros.
 *
 * All functions return SF_OK or the SF_ERR_* codes of sf.h; sf_last_error() has the text.
 *
 * REFUSALS (SF_ERR_ARG unless said otherwise; nothing launched, nothing written): a null argument; n < 0 (n == 0 is SF_OK);
 * n > 65535; rows or cols outside 1..4096, or rows * cols > 2^24; max_regions outside 0..65535 (0 means summaries and labels
 * only, and regions_out may then be NULL); z_max outside (0, 32]; b_max not finite; a negative dz_abs or dz_rel; a NaN or inf
 * in sfr_params; connectivity other than 4 or 8; min_pixels < 1; use_b other than 0 / 1; use_b with the b pointer missing; a
 * stream index out of range (the code of sf_get_current); scratch that cannot be allocated (SF_ERR_NOMEM).
 *
 * NOT HERE: tracking a region from frame to frame, 3-D boxes in metres, merging regions across a depth jump, and regions of
 * the map.
 */
#ifndef SF_REGIONS_H_
#define SF_REGIONS_H_

#include "sf.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sfr_params {
    float   z_max;         /* metres, 0 < . <= 32 */
    float   b_max;         /* finite; with use_b a pixel is in the mask when b < b_max */
    float   dz_abs;        /* metres, >= 0 */
    float   dz_rel;        /* per metre of the nearer depth, >= 0 */
    int32_t connectivity;  /* 4 or 8 */
    int32_t min_pixels;    /* >= 1 */
    int32_t use_b;         /* 0 / 1 */
    int32_t reserved;      /* not read */
} sfr_params;              /* 32 bytes; sfr_params_bytes() reports it */

typedef struct sfr_region {
    int32_t n, first, v_min, v_max, u_min, u_max, z_min, z_max;
    int64_t sum_v, sum_u, sum_z, sum_b;
} sfr_region;              /* 64 bytes; sfr_region_bytes() reports it */

typedef struct sfr_summary {
    int32_t n_mask;        /* pixels in M */
    int32_t n_components;  /* all components, small ones included */
    int32_t n_regions;     /* R */
    int32_t n_written;     /* min(R, max_regions) */
    int32_t reserved[4];   /* written as 0 */
} sfr_summary;             /* 32 bytes; sfr_summary_bytes() reports it */

int sfr_version(void); /* 1 */
size_t sfr_params_bytes(void);  /* sizeof(sfr_params) = 32 */
size_t sfr_region_bytes(void);  /* sizeof(sfr_region) = 64 */
size_t sfr_summary_bytes(void); /* sizeof(sfr_summary) = 32 */

/* z_max 8, b_max 0.5, dz_abs 0.05, dz_rel 0.02, connectivity 8, min_pixels 16, use_b 1. These are parameter defaults, NOT
 * tuned thresholds: nobody has tuned them on real data, and what counts as one moving thing is the caller's to decide. */
int sfr_default_params(sfr_params *p);

/* Pure host, no handle, no GPU: SF_OK, or SF_ERR_ARG for null parameters or ones the refusal list names. */
int sfr_check_params(const sfr_params *p);

/* Entry q < n labels the current frame of streams[q]: the level-0 depth sf_get_current returns and the image
 * sf_get_b_image returns, read on the device where they lie. params holds n entries; summaries_out is HOST memory for n
 * records, regions_out HOST memory for n * max_regions records (entry q at q * max_regions). labels_out is NULL or an array
 * of n HOST pointers (rows * cols int32 each), any of which may be NULL. Ordered on the handle's HIP stream; returns after
 * the results are in host memory. */
int sfr_label_streams(sf_handle *h, int n, const int32_t *streams, const sfr_params *params, int max_regions, sfr_summary *summaries_out,
                      sfr_region *regions_out, int32_t *const *labels_out);

/* The same with frames in HOST memory: depth[q] (and b[q]) of rows x cols, one size per call. b is an array of n pointers,
 * or NULL when no entry sets use_b; a pointer whose entry's use_b is clear is not read. */
int sfr_label_images(sf_handle *h, int rows, int cols, int n, const float *const *depth, const float *const *b, const sfr_params *params,
                     int max_regions, sfr_summary *summaries_out, sfr_region *regions_out, int32_t *const *labels_out);

/* The same with DEVICE pointers in the (host) arrays depth, b and labels_out; summaries_out and regions_out are ONE device
 * pointer each, to n and to n * max_regions records, 8-byte aligned. Asynchronous on the handle's stream; nothing is read
 * back. */
int sfr_label_images_device(sf_handle *h, int rows, int cols, int n, const void *const *depth, const void *const *b, const sfr_params *params,
                            int max_regions, void *summaries_out, void *regions_out, void *const *labels_out);

#ifdef __cplusplus
}
#endif
#endif
