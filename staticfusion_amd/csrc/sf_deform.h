// sf_deform.h — device code of include/sf_deform.h (host side: sf_hip_deform.hip; the shared rules: sf_deform_rules.h): every
// surfel of a map bound to the nodes of a deformation graph and, for an apply, deformed in place. One kernel, two forms:
//   bind    the binding of every surfel (4 indices, 4 weights) to a table the host reads back
//   apply   DEFORM of every surfel in place; per workgroup the numbers of bound and of short surfels
// A launch works on table entry blockIdx.y; grid.x is sized for the largest entry and workgroups beyond an entry's own
// extent leave at once. One lane per surfel. The workgroup stages (g, time) of SFD_TILE nodes at a time in LDS (16 bytes per
// node, 4 KB); every lane walks the tile with broadcast reads -- all lanes of a wave read the same address -- and keeps its
// best five (d2, j) in registers by ordered insertion (sfd_best_offer). The search is brute force on purpose: it is exact and
// needs no reach parameter. The lane then gathers the transforms of its nodes from global memory, blends and stores.
// Every loop is bounded by G or by a constant. There are no atomics: a workgroup's counts go to its own two words, which the
// host adds up. No workgroup waits for another one.
#pragma once
#include "sf_deform_rules.h"
#include "sf_device_common.h"

typedef int __attribute__((ext_vector_type(4))) sfd_int4;

#define SFD_BLOCK 256
#define SFD_WAVES (SFD_BLOCK / 64)
#define SFD_TILE 256  // nodes staged at a time: one per thread

struct DeformArgs {
    float *map;             // the map's buf[0]: count x 12
    int count;
    int G;                  // 1 .. SFD_MAX_NODES
    const vfloat4 *nodes;   // [G]: g.x, g.y, g.z, time
    const float *M;         // [G][12]: row-major [A | t]
    float time_window;
    int *idx_out;           // bind: [count][4]
    float *w_out;           // bind: [count][4]
    int *block_counts;      // apply: [ceil(count / SFD_BLOCK)][2]: bound, short
};

template <bool APPLY>
__global__ __launch_bounds__(SFD_BLOCK) void sfd_kernel(const DeformArgs *tab) {
    __shared__ vfloat4 tile[SFD_TILE];
    __shared__ int wcount[SFD_WAVES][2];
    const DeformArgs &a = tab[blockIdx.y];
    const int n = a.count, G = a.G;
    if ((int)blockIdx.x * SFD_BLOCK >= n) return;  // (the whole workgroup: nobody is left at a barrier)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int e = blockIdx.x * SFD_BLOCK + tid;
    const bool mine = e < n;
    vfloat4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = v0, v2 = v0;
    if (mine) {
        const auto q4 = (gptr<const vfloat4>)(as_global(a.map) + (size_t)e * 12);
        v0 = q4[0];
        v1 = q4[1];
        if (APPLY) v2 = q4[2];
    }
    const float p[3] = {v0.x, v0.y, v0.z};
    const float tau = v1.z;  // s[6], the init time
    SfdBest best;
    sfd_best_init(&best);
    for (int first = 0; first < G; first += SFD_TILE) {
        const int held = min(SFD_TILE, G - first);
        __syncthreads();  // (the tile of the round before has been read)
        if (tid < held) tile[tid] = as_global(a.nodes)[first + tid];
        __syncthreads();
        if (mine)
            for (int k = 0; k < held; k++) {
                const vfloat4 g = tile[k];
                sfd_best_offer(&best, g.x, g.y, g.z, g.w, first + k, p, tau, a.time_window);
            }
    }
    int idx[4] = {-1, -1, -1, -1};
    float w[4] = {0.f, 0.f, 0.f, 0.f};
    const int m = mine ? sfd_best_finish(&best, idx, w) : 0;
    if (!APPLY) {
        if (mine) {
            *((gptr<sfd_int4>)(as_global(a.idx_out) + (size_t)e * 4)) = sfd_int4{idx[0], idx[1], idx[2], idx[3]};
            *((gptr<vfloat4>)(as_global(a.w_out) + (size_t)e * 4)) = vfloat4{w[0], w[1], w[2], w[3]};
        }
        return;
    }
    if (m > 0) {
        float g4[12] = {}, M4[48] = {};
        for (int i = 0; i < 4; i++) {
            if (i >= m) continue;
            const int j = idx[i];  // 0 <= j < G
            const vfloat4 g = as_global(a.nodes)[j];
            g4[3 * i] = g.x;
            g4[3 * i + 1] = g.y;
            g4[3 * i + 2] = g.z;
            const auto m4 = (gptr<const vfloat4>)(as_global(a.M) + (size_t)j * 12);
            for (int r = 0; r < 3; r++) {
                const vfloat4 row = m4[r];
                M4[12 * i + 4 * r] = row.x;
                M4[12 * i + 4 * r + 1] = row.y;
                M4[12 * i + 4 * r + 2] = row.z;
                M4[12 * i + 4 * r + 3] = row.w;
            }
        }
        float s[12] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w};
        sfd_deform_core(m, w, g4, M4, s, s);
        const auto q4 = (gptr<vfloat4>)(as_global(a.map) + (size_t)e * 12);
        q4[0] = vfloat4{s[0], s[1], s[2], s[3]};
        q4[1] = vfloat4{s[4], s[5], s[6], s[7]};  // (whole lines: storing rows 0 and 2 only measured the same)
        q4[2] = vfloat4{s[8], s[9], s[10], s[11]};
    }
    const unsigned long long bound = __ballot(m > 0), few = __ballot(m > 0 && m < 4);
    if (lane == 0) {
        wcount[wave][0] = (int)__popcll(bound);
        wcount[wave][1] = (int)__popcll(few);
    }
    __syncthreads();
    if (tid == 0) {
        int b = 0, f = 0;
        for (int k = 0; k < SFD_WAVES; k++) {
            b += wcount[k][0];
            f += wcount[k][1];
        }
        a.block_counts[2 * blockIdx.x] = b;
        a.block_counts[2 * blockIdx.x + 1] = f;
    }
}
