// sf_carve.h — device code of include/sf_carve.h (host side: sf_hip_carve.hip): which surfels of a table of maps later frames saw
// through. One surfel-stationary kernel: workgroup (blockIdx.x, blockIdx.y) takes SFW_BLOCK surfels of map blockIdx.y, the grid is
// sized for the largest map and workgroups beyond their map's extent leave at once.
//
// One lane owns one surfel: it loads its 48 bytes once as three 16-byte loads (a wave reads 3 KB contiguous) and walks the
// entries of ITS map, which the host has sorted by map (first, n_entries). The entry -- t_inv, intrinsics, size, frame pointer --
// is the same for every lane of the workgroup: it is read through a uniform address, so it lives in scalar registers, and the
// frame pointer is a scalar base for the window gather (2w + 1 runs of 2w + 1 consecutive floats: the frames are column-major, so
// the inner loop of the shared rule runs down a column). The rule is the text of sf_carve_rules.h, which the host compiles too.
// The two votes stay in registers; the packed word is stored only where a vote buffer was asked for. The predicate "stays" goes
// out as the wave's ballot, written by one lane, the block's count goes through LDS, and the six counts are popcounts of ballots
// added with one integer atomic per wave and field (none for a zero): integer sums, so nothing depends on the order of arrival.
// There are no float atomics and no atomics on votes. The scan and the ordered write are those of the bounded maps
// (sf_map_window.h through sfw_launch_scan / sfw_launch_write). All loops are bounded: n_entries <= 65535, the window <= 7 x 7.
#pragma once
#include "sf_carve_rules.h"
#include "sf_device_common.h"
#include "sf_window_args.h"  // SFW_BLOCK, SFW_WAVES

#define SFE_COUNT_WORDS 8  // n_in, n_judged, n_through, n_supported, n_occluded, n_carved (this kernel), n_out (the scan), 0

struct CarveEntry {
    SfeView view;
    const float *zf;  // rows x cols column-major, device
};

struct CarveMap {
    const float *surfels;  // count x 12 (the map's buf[0])
    int count;
    int first, n_entries;  // its entries in the sorted entry table
    SfeRule rule;
    unsigned *votes;              // [count]: v_through | v_support << 16, or null
    unsigned long long *ballots;  // [ceil(count / 64)]: bit l of word w = surfel 64 w + l stays
    int *block_counts;            // [ceil(count / SFW_BLOCK)]: surfels of the block that stay
    int *counts;                  // [SFE_COUNT_WORDS], zeroed before the launch
};

__global__ __launch_bounds__(SFW_BLOCK) void sfe_carve_kernel(const CarveMap *__restrict__ mtab, const CarveEntry *__restrict__ etab) {
    __shared__ int wcount[SFW_WAVES];
    const CarveMap &a = mtab[blockIdx.y];
    const int n = a.count;
    if ((int)blockIdx.x * SFW_BLOCK >= n) return;  // a workgroup of a larger map of the batch
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int e = blockIdx.x * SFW_BLOCK + tid;
    const bool in = e < n;
    int v_through = 0, v_support = 0;
    bool judged = false, occluded = false;
    if (in) {
        const auto q4 = (gptr<const vfloat4>)(as_global(a.surfels) + (size_t)e * 12);
        const vfloat4 r0 = q4[0], r1 = q4[1], r2 = q4[2];
        const float s[12] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w};
        const SfeRule rule = a.rule;
        const int k1 = a.first + a.n_entries;
        for (int k = a.first; k < k1; k++) {  // wave-uniform trip count
            const CarveEntry &en = etab[k];
            int found[3];
            const int cls = sfe_observe_core(s, &en.view, as_global(en.zf), &rule, found);
            v_through += cls == SFE_THROUGH;
            v_support += cls == SFE_SUPPORTED;
            judged = judged || cls != SFE_UNSEEN;
            occluded = occluded || cls == SFE_OCCLUDED;
        }
        if (a.votes) as_global(a.votes)[e] = (unsigned)v_through | ((unsigned)v_support << 16);
    }
    const SfeRule rule = a.rule;
    const bool carved = in && sfe_decide_core(v_through, v_support, &rule);
    const unsigned long long stays = __ballot(in && !carved);
    const unsigned long long b[6] = {__ballot(in),         __ballot(judged),   __ballot(v_through > 0),
                                     __ballot(v_support > 0), __ballot(occluded), __ballot(carved)};
    if (lane == 0) {
        wcount[wave] = (int)__popcll(stays);
        if (blockIdx.x * SFW_BLOCK + wave * 64 < n) a.ballots[(size_t)blockIdx.x * SFW_WAVES + wave] = stays;
#pragma unroll
        for (int f = 0; f < 6; f++) {
            const int c = (int)__popcll(b[f]);
            if (c) __hip_atomic_fetch_add(as_global(a.counts) + f, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __syncthreads();
    if (tid == 0) {
        int t = 0;
        for (int w = 0; w < SFW_WAVES; w++) t += wcount[w];
        a.block_counts[blockIdx.x] = t;
    }
}
