// sf_map_window.h — device code of include/sf_map_window.h (host side: sf_hip_map_window.hip): the order-preserving (stable)
// partition of a map's 48-byte surfel records by a per-surfel predicate, for a table of maps. The selected surfels of `src`
// go to [0, k) of `dst`, the others (where somebody wants them: move_rest) to [k, count), both in their old order. Three plain launches in the shape of the clean
// stage of a fuse (sf_fusion.h: sf_clean_flag / scan / write): predicate + per-block counts, a one-workgroup scan of the
// block counts, the ordered move. No workgroup waits for another one.
#pragma once
#include "sf_device_common.h"
#include "sf_records.h"  // load_policy
#include "sf_window_args.h"  // WindowArgs, SFW_BLOCK, SFW_WAVES

// load policy of the record reads when SF_WINDOW_POLICY is not set: 0 default, 1 the move pass non-temporal, 2 both passes
#define SFW_DEFAULT_POLICY 0

// Every kernel works on table entry blockIdx.y (the scan: blockIdx.x); grid.x is sized for the largest map of the batch and
// workgroups beyond a map's own extent leave at once.

// the tests of the filter for one record: fp32, in the order the header states, no contraction (-ffp-contract=off). A
// comparison with a NaN operand is false.
__device__ __forceinline__ bool sfw_selected(const WindowArgs &a, vfloat4 pos_conf, float t_last) {
    bool s = true;
    if (a.use_conf) s = s && (pos_conf.w >= a.min_confidence);
    if (a.use_age) s = s && (a.tick - t_last <= a.max_age);
    if (a.use_radius) {
        const float dx = pos_conf.x - a.cx, dy = pos_conf.y - a.cy, dz = pos_conf.z - a.cz;
        s = s && ((dx * dx + dy * dy) + dz * dz <= a.r2);
    }
    return s != (a.invert != 0);
}

// NT: the records are read with the non-temporal policy (sf_records.h, load_policy)
template <bool NT>
__global__ __launch_bounds__(SFW_BLOCK) void sfw_flag_kernel(const WindowArgs *tab) {
    __shared__ int wcount[SFW_WAVES];
    const WindowArgs &a = tab[blockIdx.y];
    const int n = a.count;
    if ((int)blockIdx.x * SFW_BLOCK >= n) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int e = blockIdx.x * SFW_BLOCK + tid;
    bool sel = false;
    if (e < n) {
        const auto q4 = (gptr<const vfloat4>)(as_global(a.src) + (size_t)e * 12);
        const vfloat4 v0 = load_policy<NT, vfloat4>(q4);
        const vfloat4 v1 = load_policy<NT, vfloat4>(q4 + 1);
        sel = sfw_selected(a, v0, v1.w);
    }
    const unsigned long long m = __ballot(sel);
    if (lane == 0) {
        wcount[wave] = (int)__popcll(m);
        if (blockIdx.x * SFW_BLOCK + wave * 64 < n) a.ballots[(size_t)blockIdx.x * SFW_WAVES + wave] = m;
    }
    __syncthreads();
    if (tid == 0) {
        int t = 0;
        for (int w = 0; w < SFW_WAVES; w++) t += wcount[w];
        a.block_counts[blockIdx.x] = t;
    }
}
// exclusive scan of the block counts in place (one workgroup per map, 1024 counts per trip), the total into result[0]
__global__ __launch_bounds__(1024) void sfw_scan_kernel(const WindowArgs *tab) {
    const WindowArgs &a = tab[blockIdx.x];
    const int base = block_counts_scan(a.block_counts, (a.count + SFW_BLOCK - 1) / SFW_BLOCK);
    if (threadIdx.x == 0) a.result[0] = base;
}
// element e with r selected elements before it goes to r if selected, to k + (e - r) otherwise: both parts keep their order
template <bool NT>
__global__ __launch_bounds__(SFW_BLOCK) void sfw_write_kernel(const WindowArgs *tab) {
    const WindowArgs &a = tab[blockIdx.y];
    const int n = a.count;
    if ((int)blockIdx.x * SFW_BLOCK >= n) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int e = blockIdx.x * SFW_BLOCK + tid;
    const int waves_here = min(SFW_WAVES, (n - (int)blockIdx.x * SFW_BLOCK + 63) / 64);  // ballot words this block wrote
    if (wave >= waves_here) return;
    const auto words = as_global((const unsigned long long *)a.ballots) + (size_t)blockIdx.x * SFW_WAVES;
    int r = a.block_counts[blockIdx.x];
    for (int w = 0; w < wave; w++) r += (int)__popcll(words[w]);
    const unsigned long long m = words[wave];
    r += (int)__popcll(m & ((1ull << lane) - 1ull));
    if (e >= n) return;
    const bool sel = (m >> lane) & 1ull;
    if (!sel && !a.move_rest) return;
    const int k = a.result[0];
    const int pos = sel ? r : k + (e - r);
    const auto q4 = (gptr<const vfloat4>)(as_global(a.src) + (size_t)e * 12);
    const auto o4 = (gptr<vfloat4>)(as_global(a.dst) + (size_t)pos * 12);
    const vfloat4 v0 = load_policy<NT, vfloat4>(q4), v1 = load_policy<NT, vfloat4>(q4 + 1), v2 = load_policy<NT, vfloat4>(q4 + 2);
    o4[0] = v0;
    o4[1] = v1;
    o4[2] = v2;
}
