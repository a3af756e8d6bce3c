// sf_register.h — device code of include/sf_register.h (host side: sf_hip_register.hip; the rules the host and the device share:
// sf_register_rules.h): a batch of (destination map, source map, start) entries registered on the voxel tables of their
// destinations. The table of a destination is the thin table of sf_voxel_table.h, filled by its sfj_insert_kernel<true> (keys + best);
// entries that name the same destination with the same cell read one table. Three kernels follow, on the handle's stream. What
// needs a grid-wide order is a launch boundary, NO WORKGROUP EVER WAITS FOR ANOTHER, every loop is bounded by a count known at
// launch, and there is no host synchronisation between the launches.
//   sfg_init_kernel       once per call, one lane per entry: E = E0, running.
//   sfg_linearise_kernel  the hot path, once per iteration and once more at the end; entry = blockIdx.y, grid.x sized for the
//                         largest entry. A workgroup whose entry has stopped or that lies beyond its entry's extent leaves after
//                         one uniform load of the state. E as floats and the table's descriptor come through workgroup-uniform
//                         addresses. Consecutive lanes take consecutive sampled surfels, SFG_PER_THREAD per lane SFG_NT apart;
//                         a lane loads position and normal of its surfel as two 16-byte loads, walks the eight probes over plain
//                         loads of the keys (a kernel boundary lies behind the insert), takes the representative's index from
//                         `best`, gathers its position (16 bytes) and, once, after the search, its normal. The 29 sums are kept
//                         per lane in 64-bit integers (sf_p2p_system.h) and added to the entry's record by p2p_block_add
//                         (sf_p2p_device.h). n_sampled and n_outside are ballot popcounts. An entry that asked for its pairs
//                         gets them written by every linearisation; the last one stays.
//   sfg_step_kernel       one lane per entry between linearisations: p2p_step_entry (sf_p2p_device.h) and, on the last
//                         linearisation or a stop, the result. With the systems an output (`keep`) record `it` of an entry
//                         stays, otherwise its one record is cleared once it has been read.
#pragma once
#include "../../include/sf_register.h"
#include "sf_p2p_device.h"
#include "sf_register_rules.h"
#include "sf_voxel_table.h"

#define SFG_NT 256
#define SFG_PER_THREAD 4  // sampled surfels per lane
#define SFG_PER_BLOCK (SFG_NT * SFG_PER_THREAD)

enum { SFG_N_SAMPLED = 0, SFG_N_OUTSIDE = 1, SFG_ERROR = 2, SFG_COUNT_WORDS = 4 };  // the int32 counters of an entry

struct RegArgs {
    const float *src;   // the source's surfels
    int count;          // ... and their number
    int total;          // ceil(count / stride): the surfels e = t * stride, t < total
    int table;          // the entry's table: its index among the JoinArgs of the call
    SfgRule rule;
    float damping;
    int iterations, min_pairs;
    float T0[16];
    long long *systems;  // keep: I + 1 records of 32 int64, zeroed before the first launch; else one
    P2pState *state;      // set by sfg_init_kernel; its D is the header's E
    sfg_result *result;
    int *counts;         // [SFG_COUNT_WORDS], zeroed before the first launch
    int *pairs;          // [total] or null: per t the partner, SFG_NOT_PAIRED or SFG_NOT_SAMPLED
};

// the table of sf_register_rules.h over the device's thin table: plain loads through pointers to global memory
struct SfgDeviceTable {
    gptr<const unsigned long long> keys, bids;
    gptr<const vfloat4> surfels;
    int count, slots, log2_slots;
    __device__ __forceinline__ uint64_t key(uint32_t slot) const { return keys[slot]; }
    __device__ __forceinline__ uint64_t best(uint32_t slot) const { return bids[slot]; }
    __device__ __forceinline__ SfgF4 quad(int r, int which) const {
        const vfloat4 v = surfels[(size_t)r * 3 + which];
        return SfgF4{v.x, v.y, v.z, v.w};
    }
};

__global__ __launch_bounds__(64) void sfg_init_kernel(const RegArgs *etab, int n_entries) {
    const int q = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (q >= n_entries) return;
    const RegArgs &p = etab[q];
    p2p_state_init(*p.state, p.T0, 0);
}

// this launch adds to record `slot` of every entry's systems
__global__ __launch_bounds__(SFG_NT) void sfg_linearise_kernel(const JoinArgs *ttab, const RegArgs *etab, int slot, int it) {
    const RegArgs &p = etab[blockIdx.y];
    if (it > p.iterations) return;  // an entry with fewer iterations than the call's largest
    const int total = p.total;
    const int base = (int)blockIdx.x * SFG_PER_BLOCK;
    if (base >= total) return;  // a workgroup of a larger entry of the batch
    const P2pState &st = *p.state;
    if (st.done) return;
    float E[12];
#pragma unroll
    for (int k = 0; k < 12; k++) E[k] = (float)st.D[k];
    const JoinArgs &ja = ttab[p.table];
    SfgDeviceTable t;
    t.keys = as_global((const unsigned long long *)ja.keys);
    t.bids = as_global((const unsigned long long *)ja.best);
    t.surfels = (gptr<const vfloat4>)as_global(ja.fill);
    t.count = ja.fill_count;
    t.slots = ja.slots;
    t.log2_slots = ja.log2_slots;
    const SfgRule rule = p.rule;
    const auto src = (gptr<const vfloat4>)as_global(p.src);
    const auto pairs = as_global(p.pairs);
    const int tid = threadIdx.x, lane = tid & 63;
    long long acc[p2p::FIELDS];
#pragma unroll
    for (int f = 0; f < p2p::FIELDS; f++) acc[f] = 0;
    int n_sampled = 0, n_outside = 0;  // (of the wave)
    bool lost = false;
#pragma unroll 1
    for (int k = 0; k < SFG_PER_THREAD; k++) {  // (every lane makes every trip: the ballots are the whole wave's)
        const int i = base + k * SFG_NT + tid;
        bool sampled = false, outside = false;
        int partner = SFG_NOT_SAMPLED;
        if (i < total) {
            const size_t e = (size_t)i * (size_t)rule.stride;  // < count
            const vfloat4 v0 = src[e * 3];
            if (sfg_confident(rule, v0.w)) {
                const vfloat4 v2 = src[e * 3 + 2];
                const SfgPair o = sfg_pair_core(t, rule, E, SfgF4{v0.x, v0.y, v0.z, v0.w}, SfgF4{v2.x, v2.y, v2.z, v2.w});
                sampled = true;
                outside = o.outside;
                lost = lost || o.lost;
                partner = o.partner;
                if (o.partner >= 0) p2p::accumulate(acc, o.a, o.rho);
            }
            if (p.pairs) pairs[i] = partner;
        }
        n_sampled += (int)__popcll(__ballot(sampled));
        n_outside += (int)__popcll(__ballot(outside));
    }
    if (lane == 0) {
        if (n_sampled) __hip_atomic_fetch_add(p.counts + SFG_N_SAMPLED, n_sampled, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (n_outside) __hip_atomic_fetch_add(p.counts + SFG_N_OUTSIDE, n_outside, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (lost) __hip_atomic_fetch_max(p.counts + SFG_ERROR, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    p2p_block_add<SFG_NT>(acc, as_global(p.systems) + (size_t)slot * p2p::WORDS);
}

// keep != 0: the systems are an output, record `it` of every entry stays; else the one record of an entry is cleared for the
// next linearisation once it has been read. The two counts are cleared likewise: they are those of one linearisation.
__global__ __launch_bounds__(64) void sfg_step_kernel(const RegArgs *etab, int n_entries, int slot, int keep, int it) {
    const int q = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (q >= n_entries) return;
    const RegArgs &p = etab[q];
    P2pState &st = *p.state;
    if (st.done) return;
    const int n_sampled = p.counts[SFG_N_SAMPLED], n_outside = p.counts[SFG_N_OUTSIDE];
    p.counts[SFG_N_SAMPLED] = 0;
    p.counts[SFG_N_OUTSIDE] = 0;
    const P2pStop o = p2p_step_entry(st, p.systems + (size_t)slot * p2p::WORDS, keep, p.iterations, p.min_pairs, p.damping, it);
    if (!o.stopped) return;  // on to the next linearisation
    // the last linearisation of the entry, or a stop: the result, from the E the linearisation was taken at
    sfg_result r;
    for (int k = 0; k < 3; k++)
        for (int c = 0; c < 4; c++) r.T[k + 4 * c] = (float)st.D[4 * k + c];
    r.T[3] = r.T[7] = r.T[11] = 0.f;
    r.T[15] = 1.f;
    r.status = o.status;
    r.iterations_done = st.iterations_done;
    r.n_first = st.n_first;
    r.ss_first = st.ss_first;
    r.n_last = o.n;
    r.ss_last = o.ss;
    r.n_sampled = n_sampled;
    r.n_outside = n_outside;
    r.reserved[0] = r.reserved[1] = r.reserved[2] = r.reserved[3] = 0;
    *p.result = r;
    st.done = 1;
}
