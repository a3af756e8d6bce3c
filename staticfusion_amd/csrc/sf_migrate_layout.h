// sf_migrate_layout.h — the host arithmetic of stream migration (include/sf_migrate.h): the layout of an exported stream
// ("blob") and the rotation of the 5-frame ring. Plain C++ without the HIP runtime: the library's host code, the copy kernel's
// header (sf_migrate.h) and the stand-alone check tests/cpp/migrate_layout.cpp all take their numbers from here.
//
// A blob is a 64-byte header followed by the segments below, in this order. A segment starts on a multiple of 16 bytes; the
// bytes that pad a segment up to the next multiple of 16 are zero. n0 = rows * cols, n_tot = the pixels of all pyramid levels.
//   state     SFM_STATE_WORDS 32-bit words: the travelling members of StreamState (sf_migrate.h: sfm_state_offset), the
//             pose ring in age order
//   stats     sf_frame_stats
//   pyr_new depth, pyr_new intensity, pyr_pred depth, pyr_pred intensity      n_tot floats each (every level)
//   labels    n_tot bytes (every level)
//   b_img     n0 floats
//   hist_d    5 x n0 floats, age 0 (the entry the next frame overwrites) first
//   hist_i    5 x n0 floats, likewise
//   with_input only: in_depth_mm, in_filtered_mm (n0 uint16 each), in_depth_metric (n0 floats), in_color (3 n0 bytes)
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/sf.h"

#define SFM_VERSION 1
#define SFM_MAGIC 0x424d4653u  // "SFMB", little endian
#define SFM_HEADER_BYTES 64
#define SFM_STATE_WORDS 347

enum {
    SFM_SEG_STATE = 0, SFM_SEG_STATS, SFM_SEG_PYR_NEW_D, SFM_SEG_PYR_NEW_I, SFM_SEG_PYR_PRED_D, SFM_SEG_PYR_PRED_I, SFM_SEG_LABELS,
    SFM_SEG_B_IMG, SFM_SEG_HIST_D,                                  // + age 0..4
    SFM_SEG_HIST_I = SFM_SEG_HIST_D + SF_HISTORY,                   // + age 0..4
    SFM_SEG_IN_DEPTH_MM = SFM_SEG_HIST_I + SF_HISTORY, SFM_SEG_IN_FILTERED_MM, SFM_SEG_IN_DEPTH_METRIC, SFM_SEG_IN_COLOR,
    SFM_SEG_COUNT,
    SFM_SEG_COUNT_NO_INPUT = SFM_SEG_IN_DEPTH_MM
};

struct SfmHeader {  // 64 bytes
    uint32_t magic, version;
    int32_t rows, cols, levels, with_input;
    uint64_t total_bytes;
    uint32_t reserved[8];
};

struct SfmLayout {
    size_t n0, n_tot;
    int segments;                     // SFM_SEG_COUNT_NO_INPUT or SFM_SEG_COUNT
    size_t offset[SFM_SEG_COUNT + 1];  // of segment q from the start of the blob; offset[segments] = total
    size_t bytes[SFM_SEG_COUNT];       // without the padding
    size_t total;
};

static inline size_t sfm_pad16(size_t b) { return (b + 15) & ~(size_t)15; }

// level sizes as sf_create computes them; false for a geometry no handle can have
static inline bool sfm_geometry(int rows, int cols, int levels, size_t *n0, size_t *n_tot) {
    if (rows < 8 || cols < 8 || levels < 1 || levels > SF_MAX_LEVELS) return false;
    if ((rows >> (levels - 1)) < 3 || (cols >> (levels - 1)) < 3) return false;
    size_t tot = 0;
    for (int L = 0; L < levels; L++) tot += (size_t)(rows >> L) * (size_t)(cols >> L);
    *n0 = (size_t)rows * cols;
    *n_tot = tot;
    return true;
}

static inline size_t sfm_segment_bytes(int seg, size_t n0, size_t n_tot) {
    if (seg == SFM_SEG_STATE) return (size_t)SFM_STATE_WORDS * 4;
    if (seg == SFM_SEG_STATS) return sizeof(sf_frame_stats);
    if (seg >= SFM_SEG_PYR_NEW_D && seg <= SFM_SEG_PYR_PRED_I) return n_tot * 4;
    if (seg == SFM_SEG_LABELS) return n_tot;
    if (seg >= SFM_SEG_B_IMG && seg < SFM_SEG_IN_DEPTH_MM) return n0 * 4;  // b_img and the ten ring entries
    if (seg == SFM_SEG_IN_DEPTH_MM || seg == SFM_SEG_IN_FILTERED_MM) return n0 * 2;
    if (seg == SFM_SEG_IN_DEPTH_METRIC) return n0 * 4;
    if (seg == SFM_SEG_IN_COLOR) return n0 * 3;
    return 0;
}

static inline bool sfm_layout(int rows, int cols, int levels, int with_input, SfmLayout *out) {
    if (!sfm_geometry(rows, cols, levels, &out->n0, &out->n_tot)) return false;
    out->segments = with_input ? SFM_SEG_COUNT : SFM_SEG_COUNT_NO_INPUT;
    size_t at = SFM_HEADER_BYTES;
    for (int q = 0; q < SFM_SEG_COUNT; q++) {
        out->offset[q] = at;
        out->bytes[q] = q < out->segments ? sfm_segment_bytes(q, out->n0, out->n_tot) : 0;
        at += sfm_pad16(out->bytes[q]);
    }
    out->offset[SFM_SEG_COUNT] = at;
    out->total = at;
    return true;
}

// The ring (sf_residuals.h): frame im_count warps from and then overwrites slot im_count % SF_HISTORY, the oldest entry. The
// entry of age a (0 = oldest .. 4 = newest) of a stream whose next frame is im_count therefore lies in this slot; it holds for
// hist_d, hist_i and hist_T alike.
static constexpr int sfm_ring_slot(int im_count, int age) { return (im_count + age) % SF_HISTORY; }

// A stream may move between handles whose next frames are src_im_count / dst_im_count when the counts are equal, or when
// both have the residual stage running (a young stream in a mature handle would be compared with history it never had).
static inline bool sfm_counts_compatible(int src_im_count, int dst_im_count) {
    if (src_im_count < 0 || dst_im_count < 0) return false;
    return src_im_count == dst_im_count || (src_im_count >= SF_HISTORY && dst_im_count >= SF_HISTORY);
}
