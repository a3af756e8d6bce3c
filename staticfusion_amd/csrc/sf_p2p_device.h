// sf_p2p_device.h — what the three point-to-plane solvers (sf_align.h, sf_bodies.h, sf_register.h) share on the device around the
// system of sf_p2p_system.h and the step of sf_align_step.h: the state of an entry, the workgroup's reduction of the 29 sums, and
// the bookkeeping of a step kernel up to the point where each writes its own result record.
#pragma once
#include "sf_align_step.h"
#include "sf_device_common.h"

struct P2pState {  // per entry (sf_bodies.h: per region slot)
    double D[12];  // the estimate, 3 x 4 row-major
    long long n_first, ss_first;
    int done;      // 1: stopped or finished (sf_bodies.h: or a slot at or above K), the result is written
    int iterations_done;
};

// D = the upper three rows of the column-major 4 x 4 T, nothing counted yet
P2P_HD static inline void p2p_state_init(P2pState &s, const float *T, int done) {
    for (int k = 0; k < 3; k++)
        for (int c = 0; c < 4; c++) s.D[4 * k + c] = (double)T[k + 4 * c];
    s.n_first = 0;
    s.ss_first = 0;
    s.done = done;
    s.iterations_done = 0;
}

// The 29 sums of the lanes of a workgroup of NT threads, added to the system record `rec` (every thread calls it): across the
// wave with shuffles, across the waves through NT / 64 x 232 bytes of LDS, then 64-bit integer atomics at agent scope: at most
// one per field per workgroup, and none for a field whose workgroup total is 0.
template <int NT>
__device__ __forceinline__ void p2p_block_add(const long long *acc, gptr<long long> rec) {
    __shared__ long long part[NT / 64][p2p::FIELDS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int f = 0; f < p2p::FIELDS; f++) {
        const long long v = wave_sum(acc[f]);
        if (lane == 0) part[wave][f] = v;
    }
    __syncthreads();
    if (tid < p2p::FIELDS) {
        long long v = 0;
#pragma unroll
        for (int w = 0; w < NT / 64; w++) v += part[w][tid];
        if (v) __hip_atomic_fetch_add(rec + tid, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

struct P2pStop {
    bool stopped;  // false: the step was taken, on to the next linearisation; n and ss are set either way
    int status;
    long long n, ss;
};

// One lane, between two linearisations: reads the record of linearisation `it` (and clears it unless `keep`: then the record is
// an output), remembers the first n and ss, and below `iterations` takes the step unless the pairs are too few. A stop -- the
// last linearisation, FEW_PAIRS, DEGENERATE -- is left to the caller: it writes its result from st.D, the estimate the
// linearisation was taken at, and sets st.done.
__device__ __forceinline__ P2pStop p2p_step_entry(P2pState &st, long long *rec, int keep, int iterations, int min_pairs, float damping, int it) {
    int64_t w[p2p::WORDS];
    for (int f = 0; f < p2p::WORDS; f++) w[f] = f < p2p::FIELDS ? rec[f] : 0;
    if (!keep)
        for (int f = 0; f < p2p::FIELDS; f++) rec[f] = 0;
    P2pStop o{true, p2p::OK, w[0], w[1]};
    if (it == 0) {
        st.n_first = o.n;
        st.ss_first = o.ss;
    }
    if (it < iterations) {
        if (o.n < (long long)min_pairs) {
            o.status = p2p::FEW_PAIRS;
        } else {
            double Dn[12];
            o.status = sfa_step_core(w, damping, st.D, Dn);
            if (o.status == p2p::OK) {
                for (int k = 0; k < 12; k++) st.D[k] = Dn[k];
                st.iterations_done = it + 1;
                o.stopped = false;
            }
        }
    }
    return o;
}
