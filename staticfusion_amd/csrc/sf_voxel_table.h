// sf_voxel_table.h — the voxel occupancy table over a map's surfels (the key, the rank and the hash: sf_join_key.h), and the
// kernel that fills it. Two users read it: the flag kernels of sf_join.h (host side: sf_hip_join.hip) and the probes of the
// map registration (sf_register.h, sf_register_rules.h; host side: sf_hip_register.hip).
//   insert   every in-grid surfel of the set that fills the table claims the slot of its voxel (thin: and bids for it)
// Table entry blockIdx.y; grid.x is sized for the largest entry and workgroups beyond an entry's own extent leave at once. No
// workgroup waits for another one.
//
// WHAT A DECISION RESTS ON. Inside the insert kernel other workgroups write the table, so a lane decides only by the value a
// device-scope atomic returned to it (the compare-and-swap of the key, the maximum of the bid): a stale line in an L1 or in
// another XCD's L2 cannot change a result. Whoever reads the table later reads it with plain loads: a kernel boundary lies between.
// A table is a set: which lane claims a slot first changes where a key lies, never which keys are in it; and the maximum
// of the bids does not depend on their order. So the results are a function of the inputs alone.
//
// EVERY PROBE LOOP IS BOUNDED BY THE NUMBER OF SLOTS. A walk that finds neither its key nor an empty slot sets the entry's
// error word and the lane leaves; the host returns SF_ERR_STATE. The load is at most one half, so this does not happen.
#pragma once
#include "sf_device_common.h"
#include "sf_join_key.h"
#include "sf_records.h"
#include "sf_window_args.h"

#define SFJ_BLOCK SFW_BLOCK

// the counters of an entry (int32 words of its result record; word 0 is the scan's total, WindowArgs::result)
enum { SFJ_N_OUT = 0, SFJ_N_OUTSIDE = 1, SFJ_N_VOXELS = 2, SFJ_N_BELOW = 3, SFJ_N_SHARED = 4, SFJ_ERROR = 5, SFJ_COUNT_WORDS = 8 };

// (whole: the table is its first half and `counts`, the rest is the join's; two records would cost both hosts more than they save)
struct JoinArgs {
    const float *fill;  // the surfels that fill the table: the map (thin), the destination (merge)
    const float *src;   // the surfels the flag kernel examines: the map (thin), the source (merge)
    float *dst;         // merge: where the first added surfel goes, destination buffer + 12 * its count
    int fill_count, count;
    int slots, log2_slots;
    float inv;          // 1.0f / cell
    int use_conf;       // min_confidence > 0
    float min_confidence;
    int stamp;
    float T[16];        // merge: column-major, source world frame -> destination world frame
    unsigned long long *keys;     // [slots], cleared to SFJ_EMPTY
    unsigned long long *best;     // thin: [slots], cleared to 0: the highest bid of the voxel in that slot
    int *slot_of;                 // thin: [count]: the slot of the surfel's voxel, -1 outside the grid
    unsigned long long *ballots;  // [ceil(count / 64)]
    int *block_counts;            // [ceil(count / SFJ_BLOCK)]
    int *counts;                  // [SFJ_COUNT_WORDS], cleared to 0
};

// `flag` of the lanes of a wave, added to one counter by one atomic
__device__ __forceinline__ void sfj_count(int *counter, bool flag, int lane) {
    const unsigned long long m = __ballot(flag);
    if (lane == 0 && m) __hip_atomic_fetch_add(counter, (int)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// THIN: slot_of and best are written; otherwise only the keys
// (static: two host objects instantiate it, each launches and registers the copy in its own code object)
template <bool THIN>
static __global__ __launch_bounds__(SFJ_BLOCK) void sfj_insert_kernel(const JoinArgs *tab) {
    const JoinArgs &a = tab[blockIdx.y];
    const int n = a.fill_count;
    if ((int)blockIdx.x * SFJ_BLOCK >= n) return;
    const int lane = threadIdx.x & 63;
    const int e = blockIdx.x * SFJ_BLOCK + threadIdx.x;
    bool outside = false, claimed = false, lost = false;
    if (e < n) {
        const vfloat4 v0 = *((gptr<const vfloat4>)(as_global(a.fill) + (size_t)e * 12));
        uint64_t key = 0;
        int found = -1;
        if (sfj_key_of(v0.x, v0.y, v0.z, a.inv, &key)) {
            const uint32_t mask = (uint32_t)a.slots - 1u;
            uint32_t slot = sfj_first_slot(key, a.log2_slots);
            for (int step = 0; step < a.slots; step++) {
                unsigned long long seen = SFJ_EMPTY;  // the slot's value before: the compare-and-swap returns it
                const bool swapped = __hip_atomic_compare_exchange_strong(a.keys + slot, &seen, (unsigned long long)key, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                                          __HIP_MEMORY_SCOPE_AGENT);
                if (swapped || seen == key) {
                    claimed = swapped;
                    found = (int)slot;
                    break;
                }
                slot = (slot + 1u) & mask;
            }
            lost = found < 0;
            if (THIN && found >= 0)
                __hip_atomic_fetch_max(a.best + found, (unsigned long long)sfj_candidate(sfj_rank_of(v0.w), (uint32_t)e), __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
        } else {
            outside = true;
        }
        if (THIN) a.slot_of[e] = found;
    }
    sfj_count(a.counts + SFJ_N_VOXELS, claimed, lane);
    if (THIN) sfj_count(a.counts + SFJ_N_OUTSIDE, outside, lane);
    if (lost) __hip_atomic_fetch_max(a.counts + SFJ_ERROR, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
