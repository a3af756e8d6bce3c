// sf_join.h — device code of include/sf_join.h (host side: sf_hip_join.hip; the key, the rank and the hash: sf_join_key.h; the
// voxel occupancy table over a map's surfels, its JoinArgs and its insert kernel: sf_voxel_table.h): the two predicates that read
// the table, and the merge's write. A call is
//   insert   sfj_insert_kernel of sf_voxel_table.h
//   flag     thin: the winner of each voxel and every surfel outside the grid; merge: the source surfels, transformed, whose
//            voxel the destination does not occupy. Ballots and block counts in the form of sfw_flag_kernel
//   scan, move   the scan and the ordered write of sf_map_window.h (thin); the merge's move transforms what it moves
// Every kernel works on table entry blockIdx.y; grid.x is sized for the largest entry and workgroups beyond an entry's own
// extent leave at once. No workgroup waits for another one. The flag kernels read the table with plain loads: a kernel boundary
// lies behind the insert. Every probe loop is bounded by the number of slots, as sf_voxel_table.h says.
#pragma once
#include "sf_voxel_table.h"

// The scan and the ordered write are those of sf_map_window.h, launched by sfw_launch_scan / sfw_launch_write (sf_host.h): the
// host fills a WindowArgs beside every JoinArgs.
#include "sf_window_args.h"

#define SFJ_WAVES SFW_WAVES

// ballots and block counts of a flag pass, in the exact form of sfw_flag_kernel (every thread of the workgroup calls it)
__device__ __forceinline__ void sfj_publish(const JoinArgs &a, int n, bool sel) {
    __shared__ int wcount[SFJ_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long m = __ballot(sel);
    if (lane == 0) {
        wcount[wave] = (int)__popcll(m);
        if ((int)blockIdx.x * SFJ_BLOCK + wave * 64 < n) a.ballots[(size_t)blockIdx.x * SFJ_WAVES + wave] = m;
    }
    __syncthreads();
    if (tid == 0) {
        int t = 0;
        for (int w = 0; w < SFJ_WAVES; w++) t += wcount[w];
        a.block_counts[blockIdx.x] = t;
    }
}

// thin: kept = outside the grid, or the highest bid of its voxel (a lane whose walk failed has slot -1; the call fails)
__global__ __launch_bounds__(SFJ_BLOCK) void sfj_thin_flag_kernel(const JoinArgs *tab) {
    const JoinArgs &a = tab[blockIdx.y];
    const int n = a.count;
    if ((int)blockIdx.x * SFJ_BLOCK >= n) return;
    const int e = blockIdx.x * SFJ_BLOCK + threadIdx.x;
    bool sel = false;
    if (e < n) {
        const int slot = a.slot_of[e];
        sel = slot < 0 || (uint32_t)a.best[slot] == 0xFFFFFFFFu - (uint32_t)e;
    }
    sfj_publish(a, n, sel);
}

// a source surfel's position in the destination's frame; the confidence travels with it
__device__ __forceinline__ vfloat4 sfj_moved_position(const JoinArgs &a, vfloat4 v0) {
    vfloat4 o;
    o.x = sfj_transform_row(a.T, 0, v0.x, v0.y, v0.z, true);
    o.y = sfj_transform_row(a.T, 1, v0.x, v0.y, v0.z, true);
    o.z = sfj_transform_row(a.T, 2, v0.x, v0.y, v0.z, true);
    o.w = v0.w;
    return o;
}

// merge: examined in the order of the header -- confidence, transform, outside the grid, the destination's voxel
__global__ __launch_bounds__(SFJ_BLOCK) void sfj_merge_flag_kernel(const JoinArgs *tab) {
    const JoinArgs &a = tab[blockIdx.y];
    const int n = a.count;
    if ((int)blockIdx.x * SFJ_BLOCK >= n) return;
    const int lane = threadIdx.x & 63;
    const int e = blockIdx.x * SFJ_BLOCK + threadIdx.x;
    bool below = false, outside = false, shared = false, lost = false;
    if (e < n) {
        const vfloat4 v0 = *((gptr<const vfloat4>)(as_global(a.src) + (size_t)e * 12));
        if (a.use_conf && !(v0.w >= a.min_confidence)) {
            below = true;
        } else {
            const vfloat4 p = sfj_moved_position(a, v0);
            uint64_t key = 0;
            if (!sfj_key_of(p.x, p.y, p.z, a.inv, &key)) {
                outside = true;
            } else {
                const uint32_t mask = (uint32_t)a.slots - 1u;
                uint32_t slot = sfj_first_slot(key, a.log2_slots);
                lost = true;
                for (int step = 0; step < a.slots; step++) {
                    const unsigned long long seen = a.keys[slot];
                    if (seen == key || seen == SFJ_EMPTY) {
                        shared = seen == key;
                        lost = false;
                        break;
                    }
                    slot = (slot + 1u) & mask;
                }
            }
        }
    }
    sfj_count(a.counts + SFJ_N_BELOW, below, lane);
    sfj_count(a.counts + SFJ_N_OUTSIDE, outside, lane);
    sfj_count(a.counts + SFJ_N_SHARED, shared, lane);
    if (lost) __hip_atomic_fetch_max(a.counts + SFJ_ERROR, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    sfj_publish(a, n, e < n && !below && !shared && !lost);
}

// The merge's ordered write: the added surfels behind the destination's own, in source order, the position through the very
// function the flag kernel used, the normal through the upper 3 x 3, confidence, colour and radius as they are, the stamp.
__global__ __launch_bounds__(SFJ_BLOCK) void sfj_merge_move_kernel(const JoinArgs *tab) {
    const JoinArgs &a = tab[blockIdx.y];
    const int n = a.count;
    if ((int)blockIdx.x * SFJ_BLOCK >= n) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int e = blockIdx.x * SFJ_BLOCK + tid;
    if (e >= n) return;  // (its wave's ballot word exists: the wave holds e' < n)
    // the rank of the ordered write (sfw_write_kernel): selected elements before e
    const auto words = as_global((const unsigned long long *)a.ballots) + (size_t)blockIdx.x * SFJ_WAVES;
    int r = a.block_counts[blockIdx.x];
    for (int w = 0; w < wave; w++) r += (int)__popcll(words[w]);
    const unsigned long long m = words[wave];
    r += (int)__popcll(m & ((1ull << lane) - 1ull));
    if (!((m >> lane) & 1ull)) return;
    const auto q4 = (gptr<const vfloat4>)(as_global(a.src) + (size_t)e * 12);
    const auto o4 = (gptr<vfloat4>)(as_global(a.dst) + (size_t)r * 12);
    const vfloat4 v0 = q4[0], v2 = q4[2];
    vfloat4 v1 = q4[1];
    vfloat4 nrm;
    nrm.x = sfj_transform_row(a.T, 0, v2.x, v2.y, v2.z, false);
    nrm.y = sfj_transform_row(a.T, 1, v2.x, v2.y, v2.z, false);
    nrm.z = sfj_transform_row(a.T, 2, v2.x, v2.y, v2.z, false);
    nrm.w = v2.w;
    if (a.stamp >= 0) v1.z = v1.w = (float)a.stamp;
    o4[0] = sfj_moved_position(a, v0);
    o4[1] = v1;
    o4[2] = nrm;
}
