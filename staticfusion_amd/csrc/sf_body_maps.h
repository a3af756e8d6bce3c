// sf_body_maps.h — device code of include/sf_body_maps.h (host side: sf_hip_body_maps.hip; the per-surfel rules:
// sf_body_map_rules.h; key, rank and hash: sf_join_key.h): a region's pixels fused into a map of its own on a voxel grid. A call is
//   insert   every surfel of the map, MOVED ON THE FLY, claims the slot of its voxel and bids for it (rank, then index)
//   pixels   the hot path: every pixel of the region that has a pixel surfel inside the grid claims or finds the slot of its
//            voxel and bids its pixel index with an integer minimum. Lanes run down v, along memory, so the five stencil
//            loads of a wave are contiguous; a workgroup whose tile holds no pixel of the label leaves after reading its labels
//   flag     per pixel: the winner of its voxel either names itself in merge_of[representative], or is counted as a conflict,
//            or -- the voxel holds no map surfel -- is flagged for the append. Ballots and block counts in the form of
//            sfw_flag_kernel, over pixels
//   scan     the scan of sf_map_window.h over the block counts
//   ---- the host reads the counts back and tests the capacities; only then:
//   commit   move and merge in place, one lane per surfel; the ordered append of the flagged pixels behind the map's own
// Every kernel works on table entry blockIdx.y; grid.x is sized for the largest entry and workgroups beyond an entry's own
// extent leave at once. Every loop is bounded by a count known at launch. No workgroup waits for another one.
//
// WHAT A DECISION RESTS ON. Inside the insert and the pixel kernel other workgroups write the table, so a lane decides only
// by the value an agent-scope atomic returned to it (the compare-and-swap of the key); the bids are atomic maxima and minima
// whose results nobody reads inside the kernel. The flag kernel reads keys, bids and slots with plain loads: a kernel boundary
// lies between. A table is a set: which lane claims a slot first changes where a key lies, never which keys are in it; and a
// maximum or a minimum does not depend on the order of its operands. All atomics are integer. So every buffer and every
// count is a function of the inputs alone.
#pragma once
#include "sf_body_map_rules.h"
#include "sf_device_common.h"
#include "sf_join_key.h"
#include "sf_records.h"

// The scan is that of sf_map_window.h, launched by sfw_launch_scan (sf_host.h): the host fills a WindowArgs beside every
// BodyMapArgs.
#include "sf_window_args.h"

#define SFP_BLOCK SFW_BLOCK
#define SFP_WAVES SFW_WAVES
#define SFP_NO_BID 0xFFFFFFFFu

// the counters of an entry (int32 words; word 0 is the scan's total, WindowArgs::result)
enum { SFP_N_ADDED = 0, SFP_N_PIXELS = 1, SFP_N_CANDIDATES = 2, SFP_N_VOXELS = 3, SFP_N_MERGED = 4, SFP_N_CONFLICT = 5, SFP_ERROR = 6, SFP_COUNT_WORDS = 8 };

struct BodyMapArgs {
    const float *z;        // rows x cols, column-major
    const int *lab;
    const uint8_t *rgb;    // rows x cols x 3 row-major, or null: 128, 128, 128
    float *map;            // the map's buf[0]: count x 12, room for capacity
    int count, t;
    int slots, log2_slots;
    float cx, cy, fx, fy;
    float pose[16], W[16];
    float inv;             // 1.0f / cell
    float z_max, normal_dz, min_dot, conf_new, gain, max_weight, time;
    unsigned long long *keys;     // [slots], cleared to SFJ_EMPTY
    unsigned long long *best;     // [slots], cleared to 0: the highest bid of the map surfels of the voxel in that slot
    unsigned *bid;                // [slots], cleared to SFP_NO_BID: the lowest pixel index among the voxel's candidates
    int *cand_slot;               // [rows x cols]: written for the pixels of the label: the slot of the candidate's voxel, else -1
    int *merge_of;                // [count], cleared to -1: the pixel index merged into the surfel
    unsigned long long *ballots;  // [ceil(px / 64)], cleared to 0
    int *block_counts;            // [ceil(px / SFP_BLOCK) + 1], cleared to 0
    int *counts;                  // [SFP_COUNT_WORDS], cleared to 0
};

// `flag` of the lanes of a wave, added to one counter by one atomic
__device__ __forceinline__ void sfp_count(int *counter, bool flag, int lane) {
    const unsigned long long m = __ballot(flag);
    if (lane == 0 && m) __hip_atomic_fetch_add(counter, (int)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// claim or find the slot of `key` by compare-and-swap: the slot, or -1 after a walk over every slot; *claimed: this lane put it there
__device__ __forceinline__ int sfp_claim(const BodyMapArgs &a, uint64_t key, bool *claimed) {
    const uint32_t mask = (uint32_t)a.slots - 1u;
    uint32_t slot = sfj_first_slot(key, a.log2_slots);
    for (int step = 0; step < a.slots; step++) {
        unsigned long long seen = SFJ_EMPTY;  // the slot's value before: the compare-and-swap returns it
        const bool swapped = __hip_atomic_compare_exchange_strong(a.keys + slot, &seen, (unsigned long long)key, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                                  __HIP_MEMORY_SCOPE_AGENT);
        if (swapped || seen == key) {
            *claimed = swapped;
            return (int)slot;
        }
        slot = (slot + 1u) & mask;
    }
    return -1;
}

// ---- 1. insert: the moved surfels of the map ------------------------------------------------------------------------------
__global__ __launch_bounds__(SFP_BLOCK) void sfp_insert_kernel(const BodyMapArgs *tab) {
    const BodyMapArgs &a = tab[blockIdx.y];
    const int n = a.count;
    if ((int)blockIdx.x * SFP_BLOCK >= n) return;
    const int lane = threadIdx.x & 63;
    const int e = blockIdx.x * SFP_BLOCK + threadIdx.x;
    bool claimed = false, lost = false;
    if (e < n) {
        const vfloat4 v0 = *((gptr<const vfloat4>)(as_global(a.map) + (size_t)e * 12));
        const float x = sfp_row(a.W, 0, v0.x, v0.y, v0.z, true), y = sfp_row(a.W, 1, v0.x, v0.y, v0.z, true), z = sfp_row(a.W, 2, v0.x, v0.y, v0.z, true);
        uint64_t key = 0;
        if (sfj_key_of(x, y, z, a.inv, &key)) {
            const int slot = sfp_claim(a, key, &claimed);
            lost = slot < 0;
            if (slot >= 0)
                __hip_atomic_fetch_max(a.best + slot, (unsigned long long)sfj_candidate(sfj_rank_of(v0.w), (uint32_t)e), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    sfp_count(a.counts + SFP_N_VOXELS, claimed, lane);
    if (lost) __hip_atomic_fetch_max(a.counts + SFP_ERROR, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the pixel surfel of pixel i = v + u * rows, which the caller knows to carry the label: false for a border pixel or one without a normal
__device__ __forceinline__ bool sfp_surfel_of_pixel(const BodyMapArgs &a, int rows, int cols, int i, float *out) {
    const int u = i / rows, v = i - u * rows;
    if (!(v >= 1 && v <= rows - 2 && u >= 1 && u <= cols - 2)) return false;  // (all four neighbours lie inside the image)
    const auto z = as_global(a.z);
    const float z5[5] = {z[i], z[i - rows], z[i + rows], z[i - 1], z[i + 1]};
    int r = 128, g = 128, b = 128;
    if (a.rgb) {
        const auto c = as_global(a.rgb) + ((size_t)v * cols + u) * 3;
        r = c[0];
        g = c[1];
        b = c[2];
    }
    return sfp_pixel_surfel_core(z5, v, u, a.pose, a.cx, a.cy, a.fx, a.fy, r, g, b, a.z_max, a.normal_dz, a.conf_new, a.time, out);
}

// ---- 2. pixels: candidates claim or find their voxel and bid ------------------------------------------------------------------
__global__ __launch_bounds__(SFP_BLOCK) void sfp_pixel_kernel(const BodyMapArgs *tab, int rows, int cols) {
    const BodyMapArgs &a = tab[blockIdx.y];
    const int px = rows * cols;  // <= 2^24
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * SFP_BLOCK + threadIdx.x;  // v + u * rows: lanes run down v
    const bool mine = i < px && as_global(a.lab)[i] == a.t;
    if (!__syncthreads_or(mine)) return;  // no pixel of the label in this tile
    bool cand = false, lost = false;
    if (mine) {
        float s[12];
        uint64_t key = 0;
        int slot = -1;
        if (sfp_surfel_of_pixel(a, rows, cols, i, s) && sfj_key_of(s[0], s[1], s[2], a.inv, &key)) {
            cand = true;
            bool claimed = false;
            slot = sfp_claim(a, key, &claimed);
            lost = slot < 0;
            if (slot >= 0) __hip_atomic_fetch_min(a.bid + slot, (unsigned)i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        a.cand_slot[i] = slot;
    }
    sfp_count(a.counts + SFP_N_PIXELS, mine, lane);
    sfp_count(a.counts + SFP_N_CANDIDATES, cand, lane);
    if (lost) __hip_atomic_fetch_max(a.counts + SFP_ERROR, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- 3. flag: what the winner of every voxel does -----------------------------------------------------------------------------
__global__ __launch_bounds__(SFP_BLOCK) void sfp_flag_kernel(const BodyMapArgs *tab, int rows, int cols) {
    __shared__ int wcount[SFP_WAVES];
    const BodyMapArgs &a = tab[blockIdx.y];
    const int px = rows * cols;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.x * SFP_BLOCK + tid;
    const bool mine = i < px && as_global(a.lab)[i] == a.t;
    if (!__syncthreads_or(mine)) return;  // (ballots and block counts of the tile stay 0: they were cleared)
    bool add = false, merged = false, conflict = false;
    if (mine) {
        const int slot = a.cand_slot[i];
        if (slot >= 0 && a.bid[slot] == (unsigned)i) {  // the winner of its voxel
            const unsigned long long top = a.best[slot];
            if (top == 0ull) {
                add = true;  // no map surfel bid for the voxel
            } else {
                const uint32_t e = 0xFFFFFFFFu - (uint32_t)top;  // the representative
                float s[12];
                sfp_surfel_of_pixel(a, rows, cols, i, s);  // (true: the pixel is a candidate)
                const vfloat4 v2 = *((gptr<const vfloat4>)(as_global(a.map) + (size_t)e * 12) + 2);
                const float ns[3] = {sfp_row(a.W, 0, v2.x, v2.y, v2.z, false), sfp_row(a.W, 1, v2.x, v2.y, v2.z, false), sfp_row(a.W, 2, v2.x, v2.y, v2.z, false)};
                if (sfp_dot(ns, s + 8) >= a.min_dot) {
                    merged = true;
                    a.merge_of[e] = i;  // one winner per voxel, one representative per voxel: nobody else writes this word
                } else {
                    conflict = true;
                }
            }
        }
    }
    sfp_count(a.counts + SFP_N_MERGED, merged, lane);
    sfp_count(a.counts + SFP_N_CONFLICT, conflict, lane);
    const unsigned long long m = __ballot(add);
    if (lane == 0) {
        wcount[wave] = (int)__popcll(m);
        if ((int)blockIdx.x * SFP_BLOCK + wave * 64 < px) a.ballots[(size_t)blockIdx.x * SFP_WAVES + wave] = m;
    }
    __syncthreads();
    if (tid == 0) {
        int t = 0;
        for (int w = 0; w < SFP_WAVES; w++) t += wcount[w];
        a.block_counts[blockIdx.x] = t;
    }
}

// ---- 4. commit: move and merge in place ---------------------------------------------------------------------------------------
// MERGE: merge_of is read; else (sfp_move_maps) the move alone
template <bool MERGE>
__global__ __launch_bounds__(SFP_BLOCK) void sfp_move_kernel(const BodyMapArgs *tab, int rows, int cols) {
    const BodyMapArgs &a = tab[blockIdx.y];
    const int e = blockIdx.x * SFP_BLOCK + threadIdx.x;
    if (e >= a.count) return;
    const auto q4 = (gptr<vfloat4>)(as_global(a.map) + (size_t)e * 12);
    const vfloat4 v0 = q4[0], v1 = q4[1], v2 = q4[2];
    float s[12] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w};
    sfp_move_core(a.W, s, s);
    if (MERGE) {
        const int i = a.merge_of[e];
        if (i >= 0) {
            float p[12];
            sfp_surfel_of_pixel(a, rows, cols, i, p);  // (true: the flag kernel merged a candidate)
            sfp_merge_core(s, p, a.gain, a.max_weight, a.time, s);
        }
    }
    q4[0] = vfloat4{s[0], s[1], s[2], s[3]};
    q4[1] = vfloat4{s[4], s[5], s[6], s[7]};
    q4[2] = vfloat4{s[8], s[9], s[10], s[11]};
}

// ---- 5. commit: the ordered append (the rank of sfw_write_kernel, over pixels) -----------------------------------------------
__global__ __launch_bounds__(SFP_BLOCK) void sfp_append_kernel(const BodyMapArgs *tab, int rows, int cols) {
    const BodyMapArgs &a = tab[blockIdx.y];
    const int px = rows * cols;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.x * SFP_BLOCK + tid;
    if (i >= px) return;  // (its wave's ballot word exists when the wave holds a pixel)
    const auto words = as_global((const unsigned long long *)a.ballots) + (size_t)blockIdx.x * SFP_WAVES;
    const unsigned long long m = words[wave];
    if (!((m >> lane) & 1ull)) return;
    int r = a.block_counts[blockIdx.x];  // the scan's exclusive offset: flagged pixels of the blocks before
    for (int w = 0; w < wave; w++) r += (int)__popcll(words[w]);
    r += (int)__popcll(m & ((1ull << lane) - 1ull));
    float s[12];
    sfp_surfel_of_pixel(a, rows, cols, i, s);  // (true: the flag kernel flagged a candidate)
    const auto o4 = (gptr<vfloat4>)(as_global(a.map) + ((size_t)a.count + (size_t)r) * 12);
    o4[0] = vfloat4{s[0], s[1], s[2], s[3]};
    o4[1] = vfloat4{s[4], s[5], s[6], s[7]};
    o4[2] = vfloat4{s[8], s[9], s[10], s[11]};
}
