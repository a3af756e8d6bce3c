// sf_align.h — device code of include/sf_align.h (host side: sf_hip_align.hip): damped point-to-plane refinement of a batch
// of (map, candidate pose, frame) entries. The map of an entry has been drawn into its key image by the drawing stage of
// the views (sfv_draw_keys: rays, clear, splat, large sprites). Three kernels follow, table entry blockIdx.y, grids sized
// for the largest entry, workgroups beyond their entry's extent leave at once:
//   sfa_model_kernel      once per call: the winner of every pixel is evaluated again from its key (sfv_to_camera and the
//                         ray table, the expressions of surfel_fragment) into the MODEL IMAGE of the entry, 32 bytes per pixel:
//                         (M.x, M.y, M.z, drawn) and (n.x, n.y, n.z, 0). Every linearisation reads this image: a pair then
//                         costs one 32-byte gather instead of the key (8 B), the surfel (48 B) and the ray (16 B).
//   sfa_linearise_kernel  the hot path, once per iteration and once more at the end: flat over the column-major index of the
//                         strided frame pixels along lanes, the 29 sums of the system (sf_p2p_system.h: quantise,
//                         accumulate) kept per lane in 64-bit integers (products of 32-bit factors: v_mad_i64_i32) and
//                         added to the entry's record by p2p_block_add (sf_p2p_device.h).
//   sfa_step_kernel       one lane per entry between linearisations: p2p_step_entry (sf_p2p_device.h), then the result.
// An entry that has stopped or finished is marked in its P2pState (uploaded with D = I and everything else 0); its workgroups
// of later launches read that word and leave. There is no host synchronisation between the launches.
#pragma once
#include "../../include/sf_align.h"
#include "sf_p2p_device.h"
#include "sf_view_common.h"

struct AlignArgs {
    const float *depth, *b;  // rows x cols column-major; b is read only with use_b
    float dist_max, z_max, b_min, damping;
    int iterations, stride, min_pairs, use_b;
    float t0[16];            // view.pose
    vfloat4 *model;          // 2 x rows x cols: the model image
    long long *systems;      // (I + 1) records of 32 int64, zeroed before the first launch
    P2pState *state;
    sfa_result *result;
};

#define SFA_NT 256
#define SFA_PER_THREAD 4  // frame pixels per lane

__global__ __launch_bounds__(256) void sfa_model_kernel(const ViewArgs *vtab, const AlignArgs *atab) {
    const ViewArgs &a = vtab[blockIdx.y];
    const AlignArgs &p = atab[blockIdx.y];
    const int px = a.rows * a.cols;  // <= 2^24
    const int idx = (int)blockIdx.x * 256 + (int)threadIdx.x;  // j + i * rows
    if (idx >= px) return;
    const unsigned long long key = as_global(a.keys)[idx];
    vfloat4 m0 = {0.f, 0.f, 0.f, 0.f}, m1 = {0.f, 0.f, 0.f, 0.f};
    if (key != SFV_EMPTY) {
        const int s = (int)(unsigned)(key & 0xffffffffull);
        PV3 h, n;
        float rad;
        sfv_to_camera(a, s, h, n, rad);
        const vfloat4 lr = as_global(a.rays)[idx];
        const PV3 l{lr.x, lr.y, lr.z};
        const PV3 M = pmul(l, pdot(h, n) / pdot(l, n));  // `corrected` of surfel_fragment
        m0 = vfloat4{M.x, M.y, M.z, 1.f};
        m1 = vfloat4{n.x, n.y, n.z, 0.f};
    }
    as_global(p.model)[2 * (size_t)idx] = m0;
    as_global(p.model)[2 * (size_t)idx + 1] = m1;
}

__global__ __launch_bounds__(SFA_NT) void sfa_linearise_kernel(const ViewArgs *vtab, const AlignArgs *atab, int it) {
    const ViewArgs &a = vtab[blockIdx.y];
    const AlignArgs &p = atab[blockIdx.y];
    if (it > p.iterations) return;  // an entry with fewer iterations than the call's largest
    const int stride = p.stride;
    const int ny = (a.rows + stride - 1) / stride, nx = (a.cols + stride - 1) / stride;
    const int total = ny * nx;
    const int base = (int)blockIdx.x * (SFA_NT * SFA_PER_THREAD);
    if (base >= total) return;  // a workgroup of a larger entry of the batch
    const P2pState &st = *p.state;
    if (st.done) return;
    float D[12];
#pragma unroll
    for (int k = 0; k < 12; k++) D[k] = (float)st.D[k];
    const int tid = threadIdx.x;
    long long acc[p2p::FIELDS] = {};  // (not a zeroing loop: with one the compiler carries every sum through the pixel loop twice)
    const float gate = p.dist_max * p.dist_max;
#pragma unroll 1
    for (int k = 0; k < SFA_PER_THREAD; k++) {
        const int t = base + k * SFA_NT + tid;
        if (t >= total) break;
        const int xs = t / ny, ys = t - xs * ny;
        const int x = xs * stride, y = ys * stride;
        const int idx = y + x * a.rows;
        const float zf = as_global(p.depth)[idx];
        bool ok = zf > 0.f && zf <= p.z_max;
        if (p.use_b) ok = ok && as_global(p.b)[idx] > p.b_min;
        if (!ok) continue;
        const PV3 P{(((float)x - a.cx) * zf) / a.fx, (((float)y - a.cy) * zf) / a.fy, zf};
        const PV3 Q{((D[0] * P.x + D[1] * P.y) + D[2] * P.z) + D[3], ((D[4] * P.x + D[5] * P.y) + D[6] * P.z) + D[7],
                    ((D[8] * P.x + D[9] * P.y) + D[10] * P.z) + D[11]};
        if (!(Q.z >= 0.4f)) continue;
        const float fpx = (a.fx * Q.x) / Q.z + a.cx, fpy = (a.fy * Q.y) / Q.z + a.cy;
        if (!(fpx >= 0.f && fpx < (float)a.cols && fpy >= 0.f && fpy < (float)a.rows)) continue;
        const int i = (int)floorf(fpx), j = (int)floorf(fpy);  // 0 <= i < cols, 0 <= j < rows
        const size_t m = 2 * ((size_t)j + (size_t)i * a.rows);
        const vfloat4 m0 = as_global(p.model)[m];
        if (!(m0.w > 0.f)) continue;  // not drawn
        const vfloat4 m1 = as_global(p.model)[m + 1];
        const PV3 M{m0.x, m0.y, m0.z}, n{m1.x, m1.y, m1.z};
        const PV3 d = psub(Q, M);
        if (!(pdot(d, d) <= gate)) continue;
        if (!(pdot(n, n) > 0.5f)) continue;
        const float r = pdot(n, d);
        if (!(fabsf(r) <= p.dist_max)) continue;
        const PV3 c = pcross(Q, n);
        const float J[6] = {c.x, c.y, c.z, n.x, n.y, n.z};
        int ai[6], rho;
        p2p::quantise(J, r, ai, &rho);
        p2p::accumulate(acc, ai, rho);
    }
    p2p_block_add<SFA_NT>(acc, as_global(p.systems) + (size_t)it * p2p::WORDS);
}

// (the I + 1 records of an entry are an output or scratch of their own: none is ever cleared, keep = 1)
__global__ __launch_bounds__(64) void sfa_step_kernel(const AlignArgs *atab, int n_entries, int it) {
    const int q = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (q >= n_entries) return;
    const AlignArgs &p = atab[q];
    P2pState &st = *p.state;
    if (st.done) return;
    const P2pStop o = p2p_step_entry(st, p.systems + (size_t)it * p2p::WORDS, 1, p.iterations, p.min_pairs, p.damping, it);
    if (!o.stopped) return;  // on to the next linearisation
    // the last linearisation of the entry, or a stop: the result, from the D the linearisation was taken at
    sfa_result r;
    sfa_compose_pose(p.t0, st.D, r.pose);
    r.status = o.status;
    r.iterations_done = st.iterations_done;
    r.n_first = st.n_first;
    r.ss_first = st.ss_first;
    r.n_last = o.n;
    r.ss_last = o.ss;
    r.reserved[0] = r.reserved[1] = r.reserved[2] = 0;
    *p.result = r;
    st.done = 1;
}
