// sf_register.h — device code of include/sf_register.h (host side: sf_hip_register.hip; the rules the host and the device share:
// sf_register_rules.h): a batch of (destination map, source map, start) entries registered on the voxel tables of their
// destinations. The table of a destination is the thin table of sf_join.h, filled by its sfj_insert_kernel<true> (keys + best);
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
//                         per lane in 64-bit integers, reduced across the wave with shuffles, across the four waves through 928
//                         bytes of LDS, and added to the entry's record with 64-bit integer atomics at agent scope: at most once
//                         per field per workgroup, and not at all for a field whose workgroup total is 0 (the reduction of
//                         sf_align.h, which sf_bodies.h runs by region). n_sampled and n_outside are ballot popcounts. An
//                         entry that asked for its pairs gets them written by every linearisation; the last one stays.
//   sfg_step_kernel       one lane per entry between linearisations: FEW_PAIRS, the step of sf_align_step.h, the status and, on
//                         the last linearisation or a stop, the result. The `keep` of sfb_step_kernel: with the systems an
//                         output record `it` of an entry stays, otherwise its one record is cleared once it has been read.
#pragma once
#include "../../include/sf_register.h"
#include "sf_align_step.h"
#include "sf_device_common.h"
#include "sf_join_key.h"
#include "sf_records.h"
#include "sf_register_rules.h"
#include "sf_window_args.h"
// sf_join.h as it is, for JoinArgs and sfj_insert_kernel<true>. It also defines the join's other kernels, which sf_hip_join.hip
// owns: inside an unnamed namespace this object's copies are its own and are never launched. (What sf_join.h includes has been
// included above, outside the namespace.)
namespace {
#include "sf_join.h"
}

#define SFG_NT 256
#define SFG_PER_THREAD 4  // sampled surfels per lane
#define SFG_PER_BLOCK (SFG_NT * SFG_PER_THREAD)

enum { SFG_N_SAMPLED = 0, SFG_N_OUTSIDE = 1, SFG_ERROR = 2, SFG_COUNT_WORDS = 4 };  // the int32 counters of an entry

struct RegState {  // per entry; set by sfg_init_kernel
    double E[12];
    long long n_first, ss_first;
    int done;      // 1: stopped or finished, the result is written
    int iterations_done;
};

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
    RegState *state;
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

__device__ __forceinline__ long long sfg_wave_sum(long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__global__ __launch_bounds__(64) void sfg_init_kernel(const RegArgs *etab, int n_entries) {
    const int q = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (q >= n_entries) return;
    const RegArgs &p = etab[q];
    RegState &s = *p.state;
    for (int k = 0; k < 3; k++)
        for (int c = 0; c < 4; c++) s.E[4 * k + c] = (double)p.T0[k + 4 * c];
    s.n_first = 0;
    s.ss_first = 0;
    s.done = 0;
    s.iterations_done = 0;
}

// this launch adds to record `slot` of every entry's systems
__global__ __launch_bounds__(SFG_NT) void sfg_linearise_kernel(const JoinArgs *ttab, const RegArgs *etab, int slot, int it) {
    __shared__ long long part[SFG_NT / 64][SFG_FIELDS];
    const RegArgs &p = etab[blockIdx.y];
    if (it > p.iterations) return;  // an entry with fewer iterations than the call's largest
    const int total = p.total;
    const int base = (int)blockIdx.x * SFG_PER_BLOCK;
    if (base >= total) return;  // a workgroup of a larger entry of the batch
    const RegState &st = *p.state;
    if (st.done) return;
    float E[12];
#pragma unroll
    for (int k = 0; k < 12; k++) E[k] = (float)st.E[k];
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
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    long long acc[SFG_FIELDS];
#pragma unroll
    for (int f = 0; f < SFG_FIELDS; f++) acc[f] = 0;
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
                if (o.partner >= 0) sfg_accumulate(acc, o);
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
#pragma unroll
    for (int f = 0; f < SFG_FIELDS; f++) {
        const long long v = sfg_wave_sum(acc[f]);
        if (lane == 0) part[wave][f] = v;
    }
    __syncthreads();
    if (tid < SFG_FIELDS) {
        long long v = 0;
#pragma unroll
        for (int w = 0; w < SFG_NT / 64; w++) v += part[w][tid];
        if (v) __hip_atomic_fetch_add(as_global(p.systems) + (size_t)slot * SFG_SYSTEM_WORDS + tid, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// keep != 0: the systems are an output, record `it` of every entry stays; else the one record of an entry is cleared for the
// next linearisation once it has been read. The two counts are cleared likewise: they are those of one linearisation.
__global__ __launch_bounds__(64) void sfg_step_kernel(const RegArgs *etab, int n_entries, int slot, int keep, int it) {
    const int q = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (q >= n_entries) return;
    const RegArgs &p = etab[q];
    RegState &st = *p.state;
    if (st.done) return;
    long long *rec = p.systems + (size_t)slot * SFG_SYSTEM_WORDS;
    int64_t w[SFG_SYSTEM_WORDS];
    for (int f = 0; f < SFG_SYSTEM_WORDS; f++) w[f] = f < SFG_FIELDS ? rec[f] : 0;
    if (!keep)
        for (int f = 0; f < SFG_FIELDS; f++) rec[f] = 0;
    const int n_sampled = p.counts[SFG_N_SAMPLED], n_outside = p.counts[SFG_N_OUTSIDE];
    p.counts[SFG_N_SAMPLED] = 0;
    p.counts[SFG_N_OUTSIDE] = 0;
    const long long n = w[0], ss = w[1];
    if (it == 0) {
        st.n_first = n;
        st.ss_first = ss;
    }
    int status = SFG_OK;
    if (it < p.iterations) {
        if (n < (long long)p.min_pairs) {
            status = SFG_FEW_PAIRS;
        } else {
            double En[12];
            status = sfa_step_core(w, p.damping, st.E, En);
            if (status == SFA_STEP_OK) {
                for (int k = 0; k < 12; k++) st.E[k] = En[k];
                st.iterations_done = it + 1;
                return;  // on to the next linearisation
            }
        }
    }
    // the last linearisation of the entry, or a stop: the result, from the E the linearisation was taken at
    sfg_result r;
    for (int k = 0; k < 3; k++)
        for (int c = 0; c < 4; c++) r.T[k + 4 * c] = (float)st.E[4 * k + c];
    r.T[3] = r.T[7] = r.T[11] = 0.f;
    r.T[15] = 1.f;
    r.status = status;
    r.iterations_done = st.iterations_done;
    r.n_first = st.n_first;
    r.ss_first = st.ss_first;
    r.n_last = n;
    r.ss_last = ss;
    r.n_sampled = n_sampled;
    r.n_outside = n_outside;
    r.reserved[0] = r.reserved[1] = r.reserved[2] = r.reserved[3] = 0;
    *p.result = r;
    st.done = 1;
}
