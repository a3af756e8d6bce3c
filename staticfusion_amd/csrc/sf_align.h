// sf_align.h — device code of include/sf_align.h (host side: sf_hip_align.hip): damped point-to-plane refinement of a batch
// of (map, candidate pose, frame) entries. The map of an entry has been drawn into its key image by the drawing stage of
// the views (sfv_draw_keys: rays, clear, splat, large sprites). Three kernels follow, table entry blockIdx.y, grids sized
// for the largest entry, workgroups beyond their entry's extent leave at once:
//   sfa_model_kernel      once per call: the winner of every pixel is evaluated again from its key (sfv_to_camera and the
//                         ray table, the expressions of surfel_fragment) into the MODEL IMAGE of the entry, 32 bytes per pixel:
//                         (M.x, M.y, M.z, drawn) and (n.x, n.y, n.z, 0). Every linearisation reads this image: a pair then
//                         costs one 32-byte gather instead of the key (8 B), the surfel (48 B) and the ray (16 B).
//   sfa_linearise_kernel  the hot path, once per iteration and once more at the end: flat over the column-major index of the
//                         strided frame pixels along lanes, the 29 sums of sfa_system kept per lane in 64-bit integers
//                         (products of 32-bit factors: v_mad_i64_i32), reduced across the wave with shuffles, across the
//                         four waves through 928 bytes of LDS, and added to the entry's record with 64-bit integer atomics:
//                         at most once per field per workgroup, and not at all for a field whose workgroup total is 0.
//   sfa_step_kernel       one lane per entry between linearisations: FEW_PAIRS, the step of sf_align_step.h, the result.
// An entry that has stopped or finished is marked in its AlignState; its workgroups of later launches read that word and
// leave. There is no host synchronisation between the launches.
#pragma once
#include "../../include/sf_align.h"
#include "sf_align_step.h"
#include "sf_view_common.h"

struct AlignState {  // per entry, uploaded with D = I and everything else 0
    double D[12];
    long long n_first, ss_first;
    int done;        // 1: stopped or finished, the result is written
    int iterations_done;
};

struct AlignArgs {
    const float *depth, *b;  // rows x cols column-major; b is read only with use_b
    float dist_max, z_max, b_min, damping;
    int iterations, stride, min_pairs, use_b;
    float t0[16];            // view.pose
    vfloat4 *model;          // 2 x rows x cols: the model image
    long long *systems;      // (I + 1) records of 32 int64, zeroed before the first launch
    AlignState *state;
    sfa_result *result;
};

#define SFA_NT 256
#define SFA_PER_THREAD 4  // frame pixels per lane
#define SFA_FIELDS 29

__device__ __forceinline__ long long sfa_wave_sum(long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

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
    __shared__ long long part[SFA_NT / 64][SFA_FIELDS];
    const ViewArgs &a = vtab[blockIdx.y];
    const AlignArgs &p = atab[blockIdx.y];
    if (it > p.iterations) return;  // an entry with fewer iterations than the call's largest
    const int stride = p.stride;
    const int ny = (a.rows + stride - 1) / stride, nx = (a.cols + stride - 1) / stride;
    const int total = ny * nx;
    const int base = (int)blockIdx.x * (SFA_NT * SFA_PER_THREAD);
    if (base >= total) return;  // a workgroup of a larger entry of the batch
    const AlignState &st = *p.state;
    if (st.done) return;
    float D[12];
#pragma unroll
    for (int k = 0; k < 12; k++) D[k] = (float)st.D[k];
    const int tid = threadIdx.x;
    long long acc[SFA_FIELDS];
#pragma unroll
    for (int f = 0; f < SFA_FIELDS; f++) acc[f] = 0;
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
        int ai[6];
#pragma unroll
        for (int q = 0; q < 6; q++) ai[q] = (int)rintf(fminf(fmaxf(J[q], -64.f), 64.f) * 4096.f);  // |.| <= 2^18
        const int rho = (int)rintf(r * 65536.f);                                                  // |.| <= 2^16
        acc[0] += 1;
        acc[1] += (long long)rho * rho;
        int f = 8;
#pragma unroll
        for (int q = 0; q < 6; q++) {
            acc[2 + q] += (long long)ai[q] * rho;
#pragma unroll
            for (int l = q; l < 6; l++) acc[f++] += (long long)ai[q] * ai[l];
        }
    }
    const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int f = 0; f < SFA_FIELDS; f++) {
        const long long v = sfa_wave_sum(acc[f]);
        if (lane == 0) part[wave][f] = v;
    }
    __syncthreads();
    if (tid < SFA_FIELDS) {
        long long v = 0;
#pragma unroll
        for (int q = 0; q < SFA_NT / 64; q++) v += part[q][tid];
        if (v) __hip_atomic_fetch_add(as_global(p.systems) + (size_t)it * SFA_SYSTEM_WORDS + tid, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(64) void sfa_step_kernel(const AlignArgs *atab, int n_entries, int it) {
    const int q = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (q >= n_entries) return;
    const AlignArgs &p = atab[q];
    AlignState &st = *p.state;
    if (st.done) return;
    const long long *w = p.systems + (size_t)it * SFA_SYSTEM_WORDS;
    const long long n = w[0], ss = w[1];
    if (it == 0) {
        st.n_first = n;
        st.ss_first = ss;
    }
    int status = SFA_OK;
    if (it < p.iterations) {
        if (n < (long long)p.min_pairs) {
            status = SFA_FEW_PAIRS;
        } else {
            double Dn[12];
            status = sfa_step_core((const int64_t *)w, p.damping, st.D, Dn);
            if (status == SFA_STEP_OK) {
#pragma unroll
                for (int k = 0; k < 12; k++) st.D[k] = Dn[k];
                st.iterations_done = it + 1;
                return;  // on to the next linearisation
            }
        }
    }
    // the last linearisation of the entry, or a stop: the result, from the D the linearisation was taken at
    sfa_result r;
    sfa_compose_pose(p.t0, st.D, r.pose);
    r.status = status;
    r.iterations_done = st.iterations_done;
    r.n_first = st.n_first;
    r.ss_first = st.ss_first;
    r.n_last = n;
    r.ss_last = ss;
    r.reserved[0] = r.reserved[1] = r.reserved[2] = 0;
    *p.result = r;
    st.done = 1;
}
