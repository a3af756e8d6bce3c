// sf_migrate.h — device code of stream migration (include/sf_migrate.h; host side: sf_hip_migrate.hip): what moves one stream's
// persistent state between two handles, into or out of a staging block in blob layout, or back to constructor state. No frame
// kernel includes this file.
//
// What travels is everything a later frame, a getter, the prediction fill-in or a fuse reads from an earlier frame:
// the planes (byte segments, sf_migrate_layout.h) and the members of StreamState listed in sfm_state_offset. What stays
// the destination's own is everything else in StreamState: sync_epoch / sync_failed (rendezvous state of a cluster handle),
// last_slot (a record slot of THIS handle), flip / lvl0 (0 / null between launches) and prof[] / cum_* (what this handle
// solved). The struct is therefore never copied whole: the kernels write the selected members word by word.
#pragma once
#include <stddef.h>

#include "sf_device_common.h"
#include "sf_migrate_layout.h"

#define SFM_THREADS 256

// One (stream, segment) pair of a copy. kind BYTES: `bytes` bytes from src to dst, any alignment. The STATE kinds: src / dst
// are a StreamState or the packed state segment of a blob, and the pose ring is rotated from the phase of src_count to the
// phase of dst_count (a pack holds it in age order).
enum { SFM_KIND_BYTES = 0, SFM_KIND_STATE_TO_STATE, SFM_KIND_STATE_TO_PACK, SFM_KIND_PACK_TO_STATE };
struct SfmSeg {
    const void *src;
    void *dst;
    unsigned bytes;
    int kind, src_count, dst_count;
};
// One (stream, segment) pair of a reset. kind FILL: `bytes` bytes at dst, any alignment, the byte at address A being byte
// A % 4 of `pattern` (0 for every plane, 0.5f for b_img, whose base is float-aligned); CTOR: dst is a StreamState.
enum { SFM_KIND_FILL = 0, SFM_KIND_CTOR };
struct SfmFill {
    void *dst;
    unsigned bytes, pattern;
    int kind;
    float kb;
};
#define SFM_ENTRY_BYTES 32  // capacity per entry of the tables (sf_hip_migrate.hip)
static_assert(sizeof(SfmSeg) <= SFM_ENTRY_BYTES && sizeof(SfmFill) <= SFM_ENTRY_BYTES, "table entries");

// Byte offset in StreamState of word w of the packed state; the pose ring entry of age a is slot (im_count + a) % SF_HISTORY.
__host__ __device__ static inline int sfm_state_offset(int w, int im_count) {
#define SFM_MEMBER(member, words)                              \
    if (w < (words)) return (int)offsetof(StreamState, member) + 4 * w; \
    w -= (words);
    SFM_MEMBER(T, 16)
    SFM_MEMBER(twist, 6)
    SFM_MEMBER(twist_level, 6)
    SFM_MEMBER(twist_old, 6)
    SFM_MEMBER(est_cov, 36)
    SFM_MEMBER(b_segm, SF_NUM_CLUSTERS)
    SFM_MEMBER(b_prior, SF_NUM_CLUSTERS)
    SFM_MEMBER(lambda_t_w, SF_NUM_CLUSTERS)
    SFM_MEMBER(kmeans, 3 * SF_NUM_CLUSTERS)
    SFM_MEMBER(conn, SF_NUM_CLUSTERS)
    SFM_MEMBER(cluster_res, SF_NUM_CLUSTERS)
    if (w < 16 * SF_HISTORY) return (int)offsetof(StreamState, hist_T) + 4 * (16 * sfm_ring_slot(im_count, w / 16) + w % 16);
    w -= 16 * SF_HISTORY;
    SFM_MEMBER(kb, 1)
    SFM_MEMBER(last_level, 1)
    SFM_MEMBER(last_first, 1)
    SFM_MEMBER(inv_max_c, 1)
    SFM_MEMBER(inv_max_d, 1)
#undef SFM_MEMBER
    return -1;
}
static_assert(16 + 3 * 6 + 36 + 3 * SF_NUM_CLUSTERS + 3 * SF_NUM_CLUSTERS + 2 * SF_NUM_CLUSTERS + 16 * SF_HISTORY + 5 == SFM_STATE_WORDS,
              "SFM_STATE_WORDS (sf_migrate_layout.h) counts the members above");
static_assert(sizeof(StreamState) % 4 == 0, "StreamState is handled in 32-bit words");

typedef __attribute__((address_space(1))) char gchar;
typedef __attribute__((address_space(1))) const char gcchar_m;
typedef unsigned __attribute__((ext_vector_type(2))) vuint2;
typedef unsigned __attribute__((ext_vector_type(4))) vuint4;

// `units` elements of type V from s to d (both aligned for V), the blocks of grid.x striding over them: SF_LOAD_BATCH loads
// in flight per lane before the first store. Every byte is read once: the loads are non-temporal (the policy the IRLS passes
// take for bytes nobody reads again, profiles/r08a_nt_retain.txt); the stores keep the default policy -- the destination's
// next frame reads them.
template <class V>
__device__ __forceinline__ void sfm_copy_units(gcchar_m *s, gchar *d, unsigned units) {
    const unsigned stride = gridDim.x * SFM_THREADS;
    for (unsigned i = blockIdx.x * SFM_THREADS + threadIdx.x; i < units; i += stride * SF_LOAD_BATCH) {
        V v[SF_LOAD_BATCH];
#pragma unroll
        for (int q = 0; q < SF_LOAD_BATCH; q++) {
            const unsigned j = i + q * stride;
            if (j < units) v[q] = __builtin_nontemporal_load((gptr<const V>)s + j);
        }
#pragma unroll
        for (int q = 0; q < SF_LOAD_BATCH; q++) {
            const unsigned j = i + q * stride;
            if (j < units) ((gptr<V>)d)[j] = v[q];
        }
    }
}

// grid.y (and .z, beyond 32768 pairs) = the (stream, segment) pair, grid.x strides over its bytes.
// Per-stream bases are not all 16-byte aligned (labels: [batch][n_tot] bytes; the uint16 and colour planes of the input stage),
// and source and destination can be misaligned differently: a segment is copied with the widest access BOTH sides allow,
// W = the lowest set bit of (src ^ dst) up to 16 -- a byte-wise head up to the first multiple of W of the destination (the source
// is congruent), the body in W-byte units, a byte-wise tail.
__global__ __launch_bounds__(SFM_THREADS) void sfm_copy_kernel(const SfmSeg *tab, int n_pairs) {
    const int pair = blockIdx.y + gridDim.y * blockIdx.z;
    if (pair >= n_pairs) return;
    const SfmSeg sg = tab[pair];
    const int tid = threadIdx.x;
    if (sg.kind != SFM_KIND_BYTES) {
        if (blockIdx.x) return;
        gcchar_m *s = (gcchar_m *)sg.src;
        gchar *d = (gchar *)sg.dst;
        for (int w = tid; w < SFM_STATE_WORDS + 1; w += SFM_THREADS) {
            if (w == SFM_STATE_WORDS) {  // the word that pads the packed state to 16 bytes
                if (sg.kind == SFM_KIND_STATE_TO_PACK) *(gptr<uint32_t>)(d + 4 * w) = 0u;
                continue;
            }
            const int so = sg.kind == SFM_KIND_PACK_TO_STATE ? 4 * w : sfm_state_offset(w, sg.src_count);
            const int dof = sg.kind == SFM_KIND_STATE_TO_PACK ? 4 * w : sfm_state_offset(w, sg.dst_count);
            *(gptr<uint32_t>)(d + dof) = *(gptr<const uint32_t>)(s + so);
        }
        return;
    }
    const unsigned long long sa = (unsigned long long)sg.src, da = (unsigned long long)sg.dst;
    const unsigned diff = ((unsigned)(sa ^ da) | 16u) & 31u;
    const unsigned W = diff & (0u - diff);  // 1, 2, 4, 8 or 16
    const unsigned head = min(sg.bytes, (W - ((unsigned)da & (W - 1u))) & (W - 1u));
    const unsigned units = (sg.bytes - head) / W, tail = sg.bytes - head - units * W;
    gcchar_m *s = (gcchar_m *)sg.src;
    gchar *d = (gchar *)sg.dst;
    if (blockIdx.x == 0) {  // head and tail: fewer than 16 bytes each
        if ((unsigned)tid < head) d[tid] = s[tid];
        const unsigned t0 = head + units * W;
        if ((unsigned)tid < tail) d[t0 + tid] = s[t0 + tid];
    }
    s += head;
    d += head;
    switch (W) {
        case 16: sfm_copy_units<vuint4>(s, d, units); break;
        case 8: sfm_copy_units<vuint2>(s, d, units); break;
        case 4: sfm_copy_units<uint32_t>(s, d, units); break;
        case 2: sfm_copy_units<uint16_t>(s, d, units); break;
        default: sfm_copy_units<uint8_t>(s, d, units); break;
    }
}

// sfm_reset_streams: what sf_create_ex leaves for a fresh stream. Same grid as the copy.
__global__ __launch_bounds__(SFM_THREADS) void sfm_reset_kernel(const SfmFill *tab, int n_pairs) {
    const int pair = blockIdx.y + gridDim.y * blockIdx.z;
    if (pair >= n_pairs) return;
    const SfmFill f = tab[pair];
    const int tid = threadIdx.x;
    gchar *d = (gchar *)f.dst;
    if (f.kind == SFM_KIND_CTOR) {
        if (blockIdx.x) return;
        for (int w = tid; w < SFM_STATE_WORDS; w += SFM_THREADS) {
            const int off = sfm_state_offset(w, 0);
            *(gptr<uint32_t>)(d + off) = sf_ctor_state_word((size_t)off, f.kb);
        }
        return;
    }
    const unsigned da = (unsigned)(unsigned long long)f.dst;
    const unsigned head = min(f.bytes, (16u - (da & 15u)) & 15u);
    const unsigned units = (f.bytes - head) / 16u, tail = f.bytes - head - units * 16u;
    if (blockIdx.x == 0) {
        if ((unsigned)tid < head) d[tid] = (char)(f.pattern >> (8u * ((da + tid) & 3u)));
        const unsigned t0 = head + units * 16u;
        if ((unsigned)tid < tail) d[t0 + tid] = (char)(f.pattern >> (8u * ((da + t0 + tid) & 3u)));
    }
    const vuint4 v = {f.pattern, f.pattern, f.pattern, f.pattern};
    const unsigned stride = gridDim.x * SFM_THREADS;
    for (unsigned i = blockIdx.x * SFM_THREADS + tid; i < units; i += stride) ((gptr<vuint4>)(d + head))[i] = v;
}
