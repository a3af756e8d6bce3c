// sf_keyframes.h — device code of include/sf_keyframes.h (host side: sf_hip_keyframes.hip): fern codes of frames, the search
// of a keyframe database, and the store of new keyframes. Everything is integer arithmetic behind two float quantisations,
// so no result depends on an order of summation or arrival.
//
// sfk_encode_kernel<W>: one workgroup per frame. The frame's thumbnail -- n, Z and G of every cell, 12 bytes x <= 4096 cells
// -- lives in LDS and never goes to HBM. The two images are read exactly once, W floats per lane and load (W = 4, 2 or 1: the
// widest that divides the cell size and the row count and that the pointers are aligned for), lanes along v, which is along
// memory in a column-major image. An ITEM is W consecutive pixels of one column inside one cell; items are numbered down
// the columns over the gr * cell rows and gc * cell columns the grid covers, so no lane ever forms an address outside them.
// A lane walks its items (tid, tid + 256, ...) without a division (KfWalk: sf_keyframe_walk.h), keeps the next item's loads in flight while it
// quantises the current one, and adds its three partial sums to the cell with LDS atomics. Then lane t packs the ferns of
// word t, t + 256, ...: fern records from global memory, cell sums gathered from LDS, one 4-byte store per eight ferns.
//
// sfk_query_kernel: one workgroup per query, lanes along slots. The database keeps its codes word by word ([word][capacity]),
// so the lanes of a wave read consecutive addresses; the query's code is broadcast from LDS. A slot that passes the tag
// filter gets the 64-bit key (distance << 32) | slot. Keys are unique, so "the m smallest" is one well-defined answer: every
// lane keeps the m smallest keys of its own slots as a sorted list in LDS (an insertion is rare once the list has warmed up),
// and m rounds of a workgroup minimum over the list heads merge the 256 lists. One pass over the database, whatever m.
//
// sfk_store_kernel: the codes of the novel entries of an add call, from [entry][word] to the database's [word][slot].
#pragma once
#include "../../include/sf_keyframes.h"
#include "sf_device_common.h"
#include "sf_keyframe_walk.h"

struct KfFrame {
    const float *depth, *grey;  // rows x cols column-major
};

template <int W>
struct KfVec;
template <>
struct KfVec<1> {
    typedef float type;
};
template <>
struct KfVec<2> {
    typedef vfloat2 type;
};
template <>
struct KfVec<4> {
    typedef vfloat4 type;
};
__device__ __forceinline__ float kf_lane(float v, int) { return v; }
__device__ __forceinline__ float kf_lane(vfloat2 v, int j) { return v[j]; }
__device__ __forceinline__ float kf_lane(vfloat4 v, int j) { return v[j]; }

template <int W>
__global__ __launch_bounds__(SFK_NT) void sfk_encode_kernel(const KfFrame *frames, const sfk_fern *ferns, int n_ferns, int words, KfGeom g,
                                                            uint32_t *codes) {
    typedef typename KfVec<W>::type Vec;
    extern __shared__ int kf_thumb[];  // [3][cells]: n, Z, G
    const int tid = threadIdx.x;
    const int cells = g.gr * g.gc;
    for (int i = tid; i < 3 * cells; i += SFK_NT) kf_thumb[i] = 0;
    __syncthreads();
    const gptr<const float> depth = as_global(frames[blockIdx.x].depth), grey = as_global(frames[blockIdx.x].grey);
    KfWalk at;
    at.start(g, tid);
    Vec z{}, y{};
    size_t px = 0;
    bool in = at.inside(g);
    if (in) {
        px = (size_t)(at.uc * g.cell + at.ur) * (size_t)g.rows + (size_t)((at.kc * g.cpw + at.kr) * W);
        z = *(gptr<const Vec>)(depth + px);
        y = *(gptr<const Vec>)(grey + px);
    }
    while (in) {
        const int c = at.kc + at.uc * g.gr;
        const Vec zc = z, yc = y;
        at.step(g);
        in = at.inside(g);
        if (in) {  // the next item's loads go out before this item's sums
            px = (size_t)(at.uc * g.cell + at.ur) * (size_t)g.rows + (size_t)((at.kc * g.cpw + at.kr) * W);
            z = *(gptr<const Vec>)(depth + px);
            y = *(gptr<const Vec>)(grey + px);
        }
        int n = 0, Z = 0, G = 0;
#pragma unroll
        for (int j = 0; j < W; j++) {
            const float zf = kf_lane(zc, j), gf = kf_lane(yc, j);
            if (zf > 0.f) {
                n++;
                Z += (int)rintf(fminf(zf, 32.f) * 1024.f);
            }
            G += (int)rintf(fminf(fmaxf(gf, 0.f), 1.f) * 4096.f);
        }
        if (n) {
            atomicAdd(&kf_thumb[c], n);
            atomicAdd(&kf_thumb[cells + c], Z);
        }
        if (G) atomicAdd(&kf_thumb[2 * cells + c], G);
    }
    __syncthreads();
    const int a = g.cell * g.cell;
    for (int w = tid; w < words; w += SFK_NT) {
        uint32_t code = 0;
        for (int j = 0; j < 8 && w * 8 + j < n_ferns; j++) {
            const sfk_fern f = ferns[w * 8 + j];
            const int n = kf_thumb[f.cell], Z = kf_thumb[cells + f.cell], G = kf_thumb[2 * cells + f.cell];
            const uint32_t bits = (G > f.t_grey * a ? 1u : 0u) | ((n > 0 && Z > f.t_depth * n) ? 2u : 0u) | (2 * n >= a ? 4u : 0u);
            code |= bits << (4 * j);
        }
        codes[(size_t)blockIdx.x * words + w] = code;
    }
}

// the number of ferns whose nibbles differ, of eight
__device__ __forceinline__ int kf_word_distance(uint32_t a, uint32_t b) {
    uint32_t x = a ^ b;
    x |= x >> 1;
    x |= x >> 2;
    return __popc(x & 0x11111111u);
}

#define SFK_NO_KEY 0xffffffffffffffffull

__device__ __forceinline__ unsigned long long kf_wave_min(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(v, d, 64);
        v = o < v ? o : v;
    }
    return v;
}

// dynamic LDS: m lists of SFK_NT keys (list place j of lane t at [j * SFK_NT + t]), SFK_NT / 64 wave minima, the query's code
__global__ __launch_bounds__(SFK_NT) void sfk_query_kernel(const uint32_t *db_codes, const int32_t *db_tags, int capacity, int count, int words,
                                                           const uint32_t *q_codes, const int32_t *q_tags, int m, sfk_match *out) {
    extern __shared__ unsigned long long kf_keys[];
    unsigned long long *wave_min = kf_keys + (size_t)m * SFK_NT;
    uint32_t *code = (uint32_t *)(wave_min + SFK_NT / 64);
    const int tid = threadIdx.x, q = blockIdx.x;
    for (int j = 0; j < m; j++) kf_keys[j * SFK_NT + tid] = SFK_NO_KEY;
    for (int w = tid; w < words; w += SFK_NT) code[w] = q_codes[(size_t)q * words + w];
    __syncthreads();
    const int tag = q_tags[q];
    unsigned long long worst = SFK_NO_KEY;  // the lane's list place m - 1
    for (int s = tid; s < count; s += SFK_NT) {
        if (tag >= 0 && db_tags[s] != tag) continue;
        int dist = 0;
        for (int w = 0; w < words; w++) dist += kf_word_distance(db_codes[(size_t)w * capacity + s], code[w]);
        const unsigned long long key = ((unsigned long long)(unsigned)dist << 32) | (unsigned)s;
        if (key < worst) {
            int j = m - 1;
            for (; j > 0 && kf_keys[(j - 1) * SFK_NT + tid] > key; j--) kf_keys[j * SFK_NT + tid] = kf_keys[(j - 1) * SFK_NT + tid];
            kf_keys[j * SFK_NT + tid] = key;
            worst = kf_keys[(m - 1) * SFK_NT + tid];
        }
    }
    // merge: the lists are sorted, so the next smallest key of the workgroup is the smallest list head
    int head = 0;
    for (int r = 0; r < m; r++) {
        const unsigned long long mine = head < m ? kf_keys[head * SFK_NT + tid] : SFK_NO_KEY;
        const unsigned long long wm = kf_wave_min(mine);
        if ((tid & 63) == 0) wave_min[tid >> 6] = wm;
        __syncthreads();
        unsigned long long best = wave_min[0];
#pragma unroll
        for (int k = 1; k < SFK_NT / 64; k++) best = wave_min[k] < best ? wave_min[k] : best;
        if (best != SFK_NO_KEY && mine == best) head++;
        if (tid == 0) {
            sfk_match r_out;
            r_out.slot = best == SFK_NO_KEY ? -1 : (int)(unsigned)(best & 0xffffffffull);
            r_out.distance = best == SFK_NO_KEY ? -1 : (int)(best >> 32);
            out[(size_t)q * m + r] = r_out;
        }
        __syncthreads();  // wave_min is written again in the next round
    }
}

__global__ __launch_bounds__(SFK_NT) void sfk_store_kernel(const uint32_t *new_codes, const int32_t *slots, const int32_t *tags, int n, int words,
                                                           uint32_t *db_codes, int32_t *db_tags, int capacity) {
    const long long i = (long long)blockIdx.x * SFK_NT + threadIdx.x;
    if (i >= (long long)n * words) return;
    const int q = (int)(i / words), w = (int)(i - (long long)q * words);
    const int slot = slots[q];
    if (slot < 0) return;  // not novel
    db_codes[(size_t)w * capacity + slot] = new_codes[i];
    if (w == 0) db_tags[slot] = tags[q];
}
