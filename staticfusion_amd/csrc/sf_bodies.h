// sf_bodies.h — device code of include/sf_bodies.h (host side: sf_hip_bodies.hip): the rigid motion of every region of a batch
// of frame pairs. Three kernels, entry = blockIdx.y (the step: one lane per region slot), on the handle's stream. What needs a
// grid-wide order is a launch boundary, NO WORKGROUP EVER WAITS FOR ANOTHER, every loop is bounded by a count known at launch,
// and there is no host synchronisation between the launches.
//
//   sfb_model_kernel      once per call: the TARGET MODEL of frame 1, 32 bytes per pixel: (P1.x, P1.y, P1.z, has_normal) and
//                         (n.x, n.y, n.z, label1 as bits). A pair then costs one 32-byte gather. Its first workgroup of every
//                         entry also sets the entry's region states: D = D0, running for slots below K.
//   sfb_linearise_kernel  the hot path, once per iteration and once more at the end. Lanes run down v, along memory: 8 bytes per
//                         frame-0 pixel (label, depth), SFB_PB pixels per workgroup, SFB_J per lane SFB_NT apart. The D of the
//                         entry's regions sits in LDS as floats. A lane keeps the 29 sums of its region in 64-bit integers
//                         for as long as its pixels stay in one region; when some lane of the wave changes region, and at the
//                         end, the wave reduces BY REGION: one ballot per distinct label, at most 64 trips, each retiring the
//                         lanes of one label, and adds the 29 totals with one 29-lane atomic instruction to a table of the
//                         workgroup in LDS while K <= SFB_LDS_REGIONS (64 x 29 x 8 B = 14 848 B), which is flushed once with
//                         64-bit global atomics, skipping zero words; a larger K takes the atomics on the global systems
//                         directly. Both paths add the same integers. A workgroup whose tile holds no pixel of a region that
//                         is still running leaves after reading its labels.
//   sfb_step_kernel       one lane per (entry, region slot) between linearisations: p2p_step_entry (sf_p2p_device.h), and on
//                         the last linearisation or a stop the result with W (sf_body_world.h).
// The system, its quantised row and its 29 sums: sf_p2p_system.h. The state of a region slot is a P2pState (sf_p2p_device.h).
#pragma once
#include "../../include/sf_bodies.h"
#include "sf_body_world.h"
#include "sf_p2p_device.h"
#include "sf_surfel_geom.h"

#define SFB_NT 256            // threads of the model and linearise kernels
#define SFB_PB 2048           // frame-0 pixels per workgroup of the linearise kernel
#define SFB_J (SFB_PB / SFB_NT)
#define SFB_FIELDS p2p::FIELDS
#define SFB_LDS_REGIONS 64    // the LDS budget of the workgroup table
#define SFB_MAX_REGIONS 256

struct BodyArgs {
    const float *z0;   // rows x cols column-major
    const int *l0;
    const float *z1;
    const int *l1;     // or null
    const int *pairs;  // M entries, or null
    vfloat4 *model;    // 2 x rows x cols
    float cx0, cy0, fx0, fy0, cx1, cy1, fx1, fy1;
    float pose0[16], pose1[16];
    float D0[16];      // the relative transform of the two poses, column-major 4 x 4
    float dist_max, z_max, normal_dz, damping;
    int iterations, min_pairs, K, pad;
};

__device__ __forceinline__ PV3 sfb_back_project(float cx, float cy, float fx, float fy, int v, int u, float z) {
    const float du = (float)u - cx, dv = (float)v - cy;
    const float xu = du * z, yv = dv * z;
    return PV3{xu / fx, yv / fy, z};
}

// ---- 1. target model ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SFB_NT) void sfb_model_kernel(const BodyArgs *args, int rows, int cols, int M, P2pState *states) {
    const int q = blockIdx.y, tid = threadIdx.x;
    const BodyArgs &a = args[q];
    if (blockIdx.x == 0) {
        for (int t = tid; t < M; t += SFB_NT) p2p_state_init(states[(size_t)q * M + t], a.D0, t >= a.K);
    }
    if (a.K == 0) return;  // (no linearisation reads the model of an entry without regions)
    const int px = rows * cols;  // <= 2^24
    const int idx = (int)blockIdx.x * SFB_NT + tid;  // v + u * rows
    if (idx >= px) return;
    const int u = idx / rows, v = idx - u * rows;
    vfloat4 m0 = {0.f, 0.f, 0.f, 0.f};
    vfloat4 m1 = {0.f, 0.f, 0.f, __int_as_float(a.l1 ? a.l1[idx] : 0)};
    if (v >= 1 && v <= rows - 2 && u >= 1 && u <= cols - 2) {  // (all four neighbours lie inside the image)
        const float z = a.z1[idx], zl = a.z1[idx - rows], zr = a.z1[idx + rows], zu = a.z1[idx - 1], zd = a.z1[idx + 1];
        const float zm = a.z_max, dz = a.normal_dz;
        bool ok = z > 0.f && z <= zm && zl > 0.f && zl <= zm && zr > 0.f && zr <= zm && zu > 0.f && zu <= zm && zd > 0.f && zd <= zm;
        ok = ok && fabsf(zl - z) <= dz && fabsf(zr - z) <= dz && fabsf(zu - z) <= dz && fabsf(zd - z) <= dz;
        if (ok) {
            const PV3 pr = sfb_back_project(a.cx1, a.cy1, a.fx1, a.fy1, v, u + 1, zr), pl = sfb_back_project(a.cx1, a.cy1, a.fx1, a.fy1, v, u - 1, zl);
            const PV3 pd = sfb_back_project(a.cx1, a.cy1, a.fx1, a.fy1, v + 1, u, zd), pu = sfb_back_project(a.cx1, a.cy1, a.fx1, a.fy1, v - 1, u, zu);
            const PV3 c = pcross(psub(pr, pl), psub(pd, pu));
            const float cc = pdot(c, c);
            if (cc > 0.f && cc < INFINITY) {
                const float s = sqrtf(cc);
                const PV3 p = sfb_back_project(a.cx1, a.cy1, a.fx1, a.fy1, v, u, z);
                m0 = vfloat4{p.x, p.y, p.z, 1.f};
                m1.x = c.x / s;
                m1.y = c.y / s;
                m1.z = c.z / s;
            }
        }
    }
    a.model[2 * (size_t)idx] = m0;
    a.model[2 * (size_t)idx + 1] = m1;
}

// ---- 2. linearise -------------------------------------------------------------------------------------------------------
// Where the wave adds the sums of region c0 (1-based): the workgroup table, or the region's system record.
__device__ __forceinline__ void sfb_add_words(bool lds, long long *tab, long long *sys, int sys_slots, int c0, int lane, long long mine) {
    if (lane < SFB_FIELDS && mine) {
        if (lds) atomicAdd((unsigned long long *)&tab[(c0 - 1) * SFB_FIELDS + lane], (unsigned long long)mine);
        else __hip_atomic_fetch_add(sys + (size_t)(c0 - 1) * sys_slots * p2p::WORDS + lane, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// systems: sys_slots records of 32 int64 per region slot; this launch adds to record `slot` of each
__global__ __launch_bounds__(SFB_NT) void sfb_linearise_kernel(const BodyArgs *args, int rows, int cols, int M, const P2pState *states, long long *systems,
                                                               int sys_slots, int slot, int it) {
    __shared__ long long tab[SFB_LDS_REGIONS * SFB_FIELDS];
    __shared__ float Ds[SFB_MAX_REGIONS * 12];
    __shared__ int live[SFB_MAX_REGIONS];
    const int q = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const BodyArgs &a = args[q];
    const int K = a.K;
    if (it > a.iterations || K == 0) return;  // (the whole workgroup, like every return before the barriers below)
    const int px = rows * cols;
    const int base = (int)blockIdx.x * SFB_PB;
    const P2pState *st = states + (size_t)q * M;
    for (int t = tid; t < K; t += SFB_NT) live[t] = !st[t].done;
    __syncthreads();
    bool any = false;
#pragma unroll
    for (int j = 0; j < SFB_J; j++) {
        const int i = base + j * SFB_NT + tid;
        const int l = i < px ? a.l0[i] : 0;
        any = any || (l >= 1 && l <= K && live[l - 1]);
    }
    if (!__syncthreads_or(any)) return;  // no pixel of a region that is still running
    const bool lds = K <= SFB_LDS_REGIONS;
    for (int t = tid; t < K * 12; t += SFB_NT) Ds[t] = (float)st[t / 12].D[t % 12];
    if (lds)
        for (int i = tid; i < K * SFB_FIELDS; i += SFB_NT) tab[i] = 0;
    __syncthreads();
    long long *sys = systems + ((size_t)q * M * sys_slots + slot) * p2p::WORDS;  // record `slot` of region slot 0 of the entry
    const float gate = a.dist_max * a.dist_max;
    const float fcols = (float)cols, frows = (float)rows;
    int cur = 0;  // the region the lane's sums belong to, 0: none
    long long acc[SFB_FIELDS];
#pragma unroll
    for (int f = 0; f < SFB_FIELDS; f++) acc[f] = 0;
#pragma unroll 1
    for (int j = 0; j <= SFB_J; j++) {  // (trip SFB_J only reduces)
        int t = 0, rho = 0;
        int ai[6] = {0, 0, 0, 0, 0, 0};
        const int i = base + j * SFB_NT + tid;
        const int l = (j < SFB_J && i < px) ? a.l0[i] : 0;
        if (l >= 1 && l <= K && live[l - 1]) {
            const float z = a.z0[i];
            if (z > 0.f && z <= a.z_max) {
                const int u = i / rows, v = i - u * rows;
                const PV3 P = sfb_back_project(a.cx0, a.cy0, a.fx0, a.fy0, v, u, z);
                const float *D = Ds + (l - 1) * 12;
                const PV3 Q{((D[0] * P.x + D[1] * P.y) + D[2] * P.z) + D[3], ((D[4] * P.x + D[5] * P.y) + D[6] * P.z) + D[7],
                            ((D[8] * P.x + D[9] * P.y) + D[10] * P.z) + D[11]};
                if (Q.z > 0.f) {
                    const float nu = a.fx1 * Q.x, nv = a.fy1 * Q.y;
                    const float qu = nu / Q.z, qv = nv / Q.z;
                    const float uf = qu + a.cx1, vf = qv + a.cy1;
                    const float su = uf + 0.5f, sv = vf + 0.5f;
                    const float ui = floorf(su), vi = floorf(sv);
                    if (ui >= 0.f && ui < fcols && vi >= 0.f && vi < frows) {
                        const size_t at = 2 * ((size_t)(int)vi + (size_t)(int)ui * rows);  // 0 <= ui < cols, 0 <= vi < rows
                        const vfloat4 m0 = a.model[at];
                        if (m0.w > 0.f) {  // the target has a normal
                            const vfloat4 m1 = a.model[at + 1];
                            const int want = a.pairs ? a.pairs[l - 1] : 0;
                            if (want == 0 || __float_as_int(m1.w) == want) {
                                const PV3 Mp{m0.x, m0.y, m0.z}, n{m1.x, m1.y, m1.z};
                                const PV3 d = psub(Q, Mp);
                                const float r = pdot(n, d);
                                if (pdot(d, d) <= gate && fabsf(r) <= a.dist_max) {
                                    const PV3 c = pcross(Q, n);
                                    const float Jv[6] = {c.x, c.y, c.z, n.x, n.y, n.z};
                                    p2p::quantise(Jv, r, ai, &rho);
                                    t = l;
                                }
                            }
                        }
                    }
                }
            }
        }
        const bool clash = t != 0 && cur != 0 && t != cur;
        if (j == SFB_J || __ballot(clash) != 0) {  // (the whole wave) reduce by region: every trip retires the lanes of one label
            unsigned long long todo = __ballot(cur > 0);
            for (int trip = 0; trip < 64; trip++) {
                if (todo == 0) break;
                const int leader = __ffsll((long long)todo) - 1;
                const int c0 = __shfl(cur, leader, 64);
                const bool join = cur == c0;
                const unsigned long long same = __ballot(join);
                const bool single = __popcll(same) == 1;
                long long mine = 0;  // lane f ends with the total of word f
#pragma unroll
                for (int f = 0; f < SFB_FIELDS; f++) {
                    const long long v = single ? __shfl(acc[f], leader, 64) : wave_sum(join ? acc[f] : 0ll);
                    if (lane == f) mine = v;
                }
                sfb_add_words(lds, tab, sys, sys_slots, c0, lane, mine);
                todo &= ~same;
            }
            cur = 0;
#pragma unroll
            for (int f = 0; f < SFB_FIELDS; f++) acc[f] = 0;
        }
        if (t) {
            cur = t;
            p2p::accumulate(acc, ai, rho);
        }
    }
    if (lds) {
        __syncthreads();
        for (int i = tid; i < K * SFB_FIELDS; i += SFB_NT) {
            const long long v = tab[i];
            if (v) {
                const int t0 = i / SFB_FIELDS;
                __hip_atomic_fetch_add(sys + (size_t)t0 * sys_slots * p2p::WORDS + (i - t0 * SFB_FIELDS), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

// ---- 3. step ------------------------------------------------------------------------------------------------------------
// keep != 0: the systems are an output, record `it` of every region slot stays; else the one record of a slot is cleared
// for the next linearisation once it has been read.
__global__ __launch_bounds__(64) void sfb_step_kernel(const BodyArgs *args, int n_slots, int M, P2pState *states, long long *systems, int sys_slots, int slot,
                                                      int keep, sfb_motion *motions, int it) {
    const int g = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (g >= n_slots) return;
    const int q = g / M, t = g - q * M;
    const BodyArgs &a = args[q];
    if (t >= a.K) return;
    P2pState &st = states[g];
    if (st.done) return;
    const P2pStop o = p2p_step_entry(st, systems + ((size_t)g * sys_slots + slot) * p2p::WORDS, keep, a.iterations, a.min_pairs, a.damping, it);
    if (!o.stopped) return;  // on to the next linearisation
    // the last linearisation of the region, or a stop: the result, from the D the linearisation was taken at
    sfb_motion r;
    sfb_estimate_as_4x4(st.D, r.d);
    sfb_world_core(a.pose0, a.pose1, st.D, r.w);
    r.status = o.status;
    r.iterations_done = st.iterations_done;
    r.n_first = st.n_first;
    r.ss_first = st.ss_first;
    r.n_last = o.n;
    r.ss_last = o.ss;
    r.reserved[0] = r.reserved[1] = r.reserved[2] = 0;
    motions[g] = r;
    st.done = 1;
}
