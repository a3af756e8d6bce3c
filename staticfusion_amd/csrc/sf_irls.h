// sf_irls.h — the IRLS of one outer iteration (solve_irls): the factored Jacobian rows, the two streaming passes with their
// reductions, the 6 x 6 and 24 x 24 solves and the iteration tail; sf_solver.h has the map of the stage headers.
#pragma once

#include "sf_cluster.h"
#include "sf_motion_filter.h"  // solve_irls ends with solve_filter_and_update
#include "sf_records.h"
#include "sf_smallmath.h"
#include "sf_solve_shared.h"

// ---------------------------------------------------------------------------------------------
//  Factored form of the two Jacobian rows.  With
//     g1 = [-1, 0, x/d, xy/d, -(x^2/d + d),  y],  g2 = [0, -1, y/d, y^2/d + d, -xy/d, -x],  g3 = [0, 0, 1, y, -x, 0]
//  the reference's rows (FrontEnd.cpp:552-585) are  a_c = pc g1 + qc g2,  a_d = twd g3 + pd g1 + qd g2,
//  b_c = -bct, b_d = -bdt  with pc = twc dcu f/d, qc = twc dcv f/d, pd = twd ddu f/d, qd = twd ddv f/d,
//  bct = twc dct, bdt = twd ddt.  Residuals then need three 6-term dot products with the solution instead
//  of twelve row entries, and the weighted rows of pass 1 are built from (w pc, w qc, ...) directly.
//  Same mathematics, different rounding association than the reference's expression order (~1e-7
//  relative on a row entry).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float vabs(float x) { return fabsf(x); }
// The rows and residuals of the passes contract multiply-add pairs explicitly (the library is built -ffp-contract=off because
// the reference has no FMA; the linearisation, whose planes are bit-compared, has none). -DSF_ROWS_FMA=0 -- part of the
// `precise` build, libsf_hip_precise.so, together with IEEE weights -- evaluates the same expressions with separate,
// individually rounded multiplies and adds: what the contraction costs in parity is measured, not asserted.
#if SF_ROWS_FMA
__device__ __forceinline__ float vfma(float a, float b, float c) { return fmaf(a, b, c); }
#else
__device__ __forceinline__ float vfma(float a, float b, float c) { return a * b + c; }
#endif

// T = float: one pixel per lane and step (packed pixel pairs buy nothing on gfx950, §5.1 of DESIGN.md)
template <class T>
struct PixFact {
    T x, y, xd, yd, xyd, xxd, yyd;  // geometry: x, y, x/d, y/d, xy/d, x^2/d + d, y^2/d + d
    T pc, qc, pd, qd, twd, bct, bdt;
    T ac, ad;                       // RAW form only: the arguments 1 + e_c, 0.01 + e_d of the two pre-weights
};

// RAW = true: the same record WITHOUT the pre-weights: pc = dcu f/d, ..., bct = dct, bdt = ddt, twd = 1, and the arguments of the
// two reciprocal square roots in o.ac / o.ad -- for pass 1, which folds each pre-weight into the Cauchy weight of its row (below)
template <class T, bool RAW = false>
__device__ __forceinline__ void fact_from_record(const LevelGeom &g, T fu, T fv, T dn, T dw, T dcu_, T dcv_, T dct_, T ddu_,
                                                 T ddv_, PixFact<T> &o) {
    const T xn = (g.inv_f_pyr * (fu - g.disp_u_i)) * dn;
    const T yn = (g.inv_f_pyr * (fv - g.disp_v_i)) * dn;
    T xw, yw;
    if (g.first) {
        xw = (g.inv_f_pyr * (fu - g.disp_u_i)) * dw;
        yw = (g.inv_f_pyr * (fv - g.disp_v_i)) * dw;
    } else {
        xw = (fu - g.disp_u_i) * dw * g.inv_f_w;
        yw = (fv - g.disp_v_i) * dw * g.inv_f_w;
    }
    const T d = 0.5f * (dn + dw);
    o.x = 0.5f * (xn + xw);
    o.y = 0.5f * (yn + yw);
    const T ddt_ = dn - dw;
    const T error_l_c = 10.f * (vabs(dct_) + vabs(dcu_) + vabs(dcv_));
    const T error_l_d = 200.f * (vabs(ddt_) + vabs(ddu_) + vabs(ddv_));
    const T inv_d = vrcpw(d);
    const T fd = g.f_inv * inv_d;
    if constexpr (RAW) {
        o.ac = 1.f + error_l_c;
        o.ad = 0.01f + error_l_d;
        o.twd = 1.f;
        o.pc = dcu_ * fd;
        o.qc = dcv_ * fd;
        o.pd = ddu_ * fd;
        o.qd = ddv_ * fd;
        o.bct = dct_;
        o.bdt = ddt_;
    } else {
        const T twc = (g.inv_max_c * vrsq(1.f + error_l_c)) * g.kph;
        o.twd = g.inv_max_d * vrsq(0.01f + error_l_d);
        o.pc = twc * (dcu_ * fd);
        o.qc = twc * (dcv_ * fd);
        o.pd = o.twd * (ddu_ * fd);
        o.qd = o.twd * (ddv_ * fd);
        o.bct = twc * dct_;
        o.bdt = o.twd * ddt_;
    }
    o.xd = o.x * inv_d;
    o.yd = o.y * inv_d;
    o.xyd = o.xd * o.y;
    o.xxd = vfma(o.xd, o.x, d);
    o.yyd = vfma(o.yd, o.y, d);
}

// residuals res = A Var - B of both rows through s1 = g1.Var, s2 = g2.Var, s3 = g3.Var
template <class T>
__device__ __forceinline__ void fact_residuals(const PixFact<T> &p, const float (&V)[6], T &res_c, T &res_d) {
    const T s1 = vfma(p.y, V[5], vfma(-p.xxd, V[4], vfma(p.xyd, V[3], vfma(p.xd, V[2], -V[0]))));
    const T s2 = vfma(-p.x, V[5], vfma(-p.xyd, V[4], vfma(p.yyd, V[3], vfma(p.yd, V[2], -V[1]))));
    const T s3 = vfma(-p.x, V[4], vfma(p.y, V[3], V[2]));
    res_c = vfma(p.pc, s1, vfma(p.qc, s2, p.bct));
    res_d = vfma(p.pd, s1, vfma(p.qd, s2, vfma(p.twd, s3, p.bdt)));
}

// A pixel that is not in validPixels gets a harmless stand-in record (finite rows) and weight 0,
// so the streaming loops are branch-free: no exec-mask juggling around the 27 accumulators.
template <int VEC>
__device__ __forceinline__ bool sanitize(RecVec<VEC> &r, int j) {
    const bool ok = r.v[R_DW][j] > 0.f;  // the linearisation stores -dw (or -0) outside validPixels
    r.dn[j] = ok ? r.dn[j] : 1.f;
    r.v[R_DW][j] = ok ? r.v[R_DW][j] : 1.f;
    // the four gradients and dct of such a pixel are stored as 0 by the linearisation (dct keeps its value in the debug-plane
    // mode only): nothing to do for them here
    r.lab[j] = ok ? (int)((j ? r.labraw >> 8 : r.labraw) & 255u) : 0;
    return ok;
}

// ---------------------------------------------------------------------------------------------
//  solveOdometryAndSegmJoint (reference FrontEnd.cpp:513-692), split into separately compiled
//  pieces so that each streaming pass gets its own register allocation.
// ---------------------------------------------------------------------------------------------
struct IrlsCtx {
    RecPtrs rp;
    LevelGeom g;
    int n;       // end of the pixel range of this workgroup (the level size in the product)
    int begin;   // start of the range (0 in the product; tools/pass_microbench.py --slices splits a level)
    int N;       // valid pixels
};

__device__ __forceinline__ IrlsCtx make_irls_ctx(const KArgs &a, int b, int L, const LDS SolveShared &s) {
    IrlsCtx c;
    const size_t rb = (size_t)uniform_i(s.rec_slot) * a.n0;
#pragma unroll
    for (int q = 0; q < R_COUNT; q++) c.rp.p[q] = uniform_ptr((gcfloat *)(a.rec[q] + rb));
    c.rp.dnew = uniform_ptr((gcfloat *)pyr_level(a, b, 0, 0, L));
    c.rp.lab = uniform_ptr((gcu8 *)(a.rec_lab + rb));
    c.rp.with_labels = uniform_i(a.p.segmentation_enabled);
    c.n = uniform_i(s.px_end);
    c.begin = uniform_i(s.px_begin);
    c.N = uniform_i(s.n_valid);
    const int rows_i = a.lrows[L], cols_i = a.lcols[L];
    const float f = float(cols_i) / (2.f * a.tan_half_fovh);
    c.g.rows_i = rows_i;
    c.g.inv_rows = 1.f / float(rows_i);
    c.g.disp_u_i = 0.5f * float(cols_i - 1);
    c.g.disp_v_i = 0.5f * float(rows_i - 1);
    c.g.inv_f_pyr = 2.f * a.tan_half_fovh / float(cols_i);
    c.g.inv_f_w = 1.f / f;
    c.g.f_inv = f;
    c.g.kph = a.p.k_photometric_res;
    c.g.inv_max_c = uniform_f(s.inv_max_c);
    c.g.inv_max_d = uniform_f(s.inv_max_d);
    c.g.first = uniform_i(s.first);
    return c;
}

// pass 1: Cauchy x b weights, 21+6 normal-equation sums (reference :615-641) -> s.red[wave][0..26]
// VAR: 0 = product code; 1 = loads only; 2 = rows + weights, no accumulation (ablation builds for
// tools/pass_microbench.py; the product always instantiates VAR 0)
//
// Scalar fp32 per pixel: on gfx950 a v_pk_*_f32 and a v_fma_f64 both cost two v_fma_f32 issue slots
// (tools/micro/valu_rate.hip), so packing buys nothing and costs registers. The 27 sums are kept
// per lane in fp32 (each lane sees <= 2 x 300 terms at QVGA level 0; the reference accumulates the
// whole sum in fp32, FrontEnd.cpp:640-641) and the 256 lanes are combined in fp64. The record of
// the next pixel pair is in flight while the current one is evaluated.
__device__ __forceinline__ void accum_row(float (&acc)[27], const float (&aw)[7]) {
    acc[0] = fmaf(aw[0], aw[0], acc[0]);    acc[1] = fmaf(aw[0], aw[1], acc[1]);
    acc[2] = fmaf(aw[0], aw[2], acc[2]);    acc[3] = fmaf(aw[0], aw[3], acc[3]);
    acc[4] = fmaf(aw[0], aw[4], acc[4]);    acc[5] = fmaf(aw[0], aw[5], acc[5]);
    acc[6] = fmaf(aw[1], aw[1], acc[6]);    acc[7] = fmaf(aw[1], aw[2], acc[7]);
    acc[8] = fmaf(aw[1], aw[3], acc[8]);    acc[9] = fmaf(aw[1], aw[4], acc[9]);
    acc[10] = fmaf(aw[1], aw[5], acc[10]);  acc[11] = fmaf(aw[2], aw[2], acc[11]);
    acc[12] = fmaf(aw[2], aw[3], acc[12]);  acc[13] = fmaf(aw[2], aw[4], acc[13]);
    acc[14] = fmaf(aw[2], aw[5], acc[14]);  acc[15] = fmaf(aw[3], aw[3], acc[15]);
    acc[16] = fmaf(aw[3], aw[4], acc[16]);  acc[17] = fmaf(aw[3], aw[5], acc[17]);
    acc[18] = fmaf(aw[4], aw[4], acc[18]);  acc[19] = fmaf(aw[4], aw[5], acc[19]);
    acc[20] = fmaf(aw[5], aw[5], acc[20]);
    acc[21] = fmaf(aw[0], aw[6], acc[21]);  acc[22] = fmaf(aw[1], aw[6], acc[22]);
    acc[23] = fmaf(aw[2], aw[6], acc[23]);  acc[24] = fmaf(aw[3], aw[6], acc[24]);
    acc[25] = fmaf(aw[4], aw[6], acc[25]);  acc[26] = fmaf(aw[5], aw[6], acc[26]);
}

// sum of v over the lane's group of P1_GROUP lanes (every lane of the group ends up with the same bits: the two / four
// exchange steps are symmetric). All 64 lanes must be active.
__device__ __forceinline__ float p1_group_sum(float v) {
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xf, 0xf, false));  // quad_perm [1,0,3,2]
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xf, 0xf, false));  // quad_perm [2,3,0,1]
    if constexpr (P1_GROUP == 16) {
        v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xf, 0xf, false));  // row_half_mirror
        v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xf, 0xf, false));  // row_mirror
    }
    return v;
}
__device__ __forceinline__ void p1_flush(float (&acc)[27], LDS SolveShared &s, int set, bool leader) {
#pragma unroll
    for (int q = 0; q < 27; q++) acc[q] = p1_group_sum(acc[q]);
    if (leader) {  // the set belongs to this lane group alone: plain read-modify-writes, one exec-mask change for all 27
#pragma unroll
        for (int q = 0; q < 27; q++) s.p1[q][set] += (double)acc[q];
    }
#pragma unroll
    for (int q = 0; q < 27; q++) acc[q] = 0.f;
}

// The load policy of a sweep, per trip. A sweep of a pass over [begin, n) is `trips` trips of SF_NT pixel
// pairs. The records of the last trips it walks -- window_px pixels, rounded up to whole trips -- are what the next pass starts on
// (serpentine order, solve_irls): they are loaded with the default policy and stay in the memory-side cache. Everything before
// them will not be read again until the cache has turned over many times: those trips are loaded non-temporally, so that they do
// not evict the windows of the other workgroups. The policy belongs to the trip whose record is LOADED: trip t issues the load of
// trip t + 1. window_px = 0: every record nt; window_px >= the range: every load default (what the passes did before there was a
// policy). The compiler merges the two arms of a branch between an nt and a plain load of one address and drops the nt bit, so a
// sweep is two instances of its loop, one per policy, entered one after the other with the same running state: the visiting order,
// the trip counts and the order of every sum are those of one loop.
//   nt_first: the record of trip 0 is loaded nt;  nt_next: trips [0, nt_next) load their successor's record nt
__device__ __forceinline__ void pass_division(int begin, int n, int window_px, bool &nt_first, int &nt_next) {
    const int trips = (((n - begin + 1) >> 1) + SF_NT - 1) / SF_NT;
    const int wtrips = (int)min((unsigned)trips, ((unsigned)max(window_px, 0) + (SF_NT * 2 - 1)) / (unsigned)(SF_NT * 2));
    const int split = trips - wtrips;  // trips [0, split) are loaded nt, [split, trips) with the default policy
    nt_first = split > 0;
    nt_next = (split >= trips) ? trips : max(split - 1, 0);
}

// the record of a sweep's first trip, with the sweep's first policy. The empty asm statements keep the two arms apart: the compiler
// otherwise hoists the loads out of the branch as ONE plain load (the nt bit is metadata it drops when it merges instructions).
// The wait that follows is where the loops expect the record: with it in front of them, the only waits inside a loop are those
// for the record it loads itself (vmcnt(2) / vmcnt(0) at the end of a trip).
#define SF_WAIT_VMCNT0 0x0F70  // s_waitcnt vmcnt(0), the other counters at their maximum (gfx9 encoding)
__device__ __forceinline__ void load_first_rec(const RecPtrs &rp, int idx0, bool nt, RecVec<2> &r) {
    if (nt) {
        asm volatile("" ::: "memory");
        load_rec<2, true>(rp, idx0, r);
        asm volatile("" ::: "memory");
    } else {
        load_rec<2, false>(rp, idx0, r);
    }
}

// what the trips of pass 1 read and never change
struct P1Consts {
    float inv_c_Cauchy, fold_kc, fold_kd, fold_gc, fold_gd;
    float Vr[6];
    int last, set;
    bool leader;
};
// the trips of pass 1 from (i0, iw) until the wave's iw reaches iw_end; NT: the policy of the record each trip loads (the next one's)
template <int VAR, bool NT>
__device__ __forceinline__ void p1_trips(const IrlsCtx &c, LDS SolveShared &s, const P1Consts &k, int iw_end, int &i0, int &iw, RecVec<2> &rv,
                                         float (&acc)[27], int &since) {
    RecVec<2> nx;
    for (; iw < iw_end; i0 += SF_NT * 2, iw += SF_NT * 2) {
        load_rec<2, NT>(c.rp, min(i0 + SF_NT * 2, k.last), nx);
        const bool in = i0 < c.n;
        const bool ok0 = sanitize<2>(rv, 0) && in, ok1 = sanitize<2>(rv, 1) && in;
        if constexpr (VAR == 1) {
            float t = rv.dn[0] + rv.dn[1];
#pragma unroll
            for (int q = 0; q < R_COUNT; q++) t += rv.v[q][0] + rv.v[q][1];
            acc[0] += t;
            rv = nx;
            continue;
        }
        float bseg0 = s.b_segm[rv.lab[0]], bseg1 = s.b_segm[rv.lab[1]];  // invalid pixels carry label 0 after sanitize()
        float fu0, fv0;
        split_index(c.g, min(i0, k.last), fu0, fv0);
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const bool ok = j ? ok1 : ok0;
            float fu = fu0, fv = fv0;
            if (j) {  // the pair may straddle a column at the odd-sized coarse levels
                const bool wrap = (fv0 + 1.f) >= (float)c.g.rows_i;
                fu = wrap ? fu0 + 1.f : fu0;
                fv = wrap ? 0.f : fv0 + 1.f;
            }
            PixFact<float> p;
#if SF_P1_FOLD
            // The weight a row finally carries is (pre-weight) x (Cauchy weight) = k rsq(a) b rsq(1 + (k rsq(a) R / c)^2) with R the
            // residual of the UNWEIGHTED row, a = 1 + e_c (0.01 + e_d) and k = kph / max (1 / max): that is b k rsq(a + (k R / c)^2) --
            // one reciprocal square root per row instead of two, and the rows are scaled once instead of twice. Same mathematics;
            // the rounding of a row entry moves by ~1e-7 relative like the factored rows themselves (pass 2 and the debug
            // expansion of the rows keep the two-step form).
            fact_from_record<float, true>(c.g, fu, fv, rv.dn[j], rv.v[R_DW][j], rv.v[R_DCU][j], rv.v[R_DCV][j], rv.v[R_DCT][j],
                                          rv.v[R_DDU][j], rv.v[R_DDV][j], p);
            if (j == 0) asm volatile("" : "+v"(bseg0), "+v"(bseg1));  // LDS reads stay unconditional, landed by now
            const float b_weight = ok ? std_max(0.f, std_min(1.f, j ? bseg1 : bseg0)) : 0.f;
            float raw_c, raw_d;
            fact_residuals<float>(p, k.Vr, raw_c, raw_d);
            const float uc = raw_c * k.fold_gc, ud = raw_d * k.fold_gd;
            const float w_c = (b_weight * k.fold_kc) * vrsq(fmaf(uc, uc, p.ac));
            const float w_d = (b_weight * k.fold_kd) * vrsq(fmaf(ud, ud, p.ad));
#else
            fact_from_record<float>(c.g, fu, fv, rv.dn[j], rv.v[R_DW][j], rv.v[R_DCU][j], rv.v[R_DCV][j], rv.v[R_DCT][j],
                                    rv.v[R_DDU][j], rv.v[R_DDV][j], p);
            if (j == 0) asm volatile("" : "+v"(bseg0), "+v"(bseg1));  // LDS reads stay unconditional, landed by now
            const float b_weight = ok ? std_max(0.f, std_min(1.f, j ? bseg1 : bseg0)) : 0.f;
            float res_c, res_d;
            fact_residuals<float>(p, k.Vr, res_c, res_d);
            const float tc = res_c * k.inv_c_Cauchy, td = res_d * k.inv_c_Cauchy;
#if SF_FAST_WEIGHTS
            const float w_c = b_weight * vrsq(vfma(tc, tc, 1.f));
            const float w_d = b_weight * vrsq(vfma(td, td, 1.f));
#else
            const float w_c = b_weight * vrsq(1.f + tc * tc);
            const float w_d = b_weight * vrsq(1.f + td * td);
#endif
#endif
            float aw[7];
            {
                const float P = w_c * p.pc, Q = w_c * p.qc;
                aw[0] = -P;
                aw[1] = -Q;
                aw[2] = vfma(P, p.xd, Q * p.yd);
                aw[3] = vfma(P, p.xyd, Q * p.yyd);
                aw[4] = -vfma(P, p.xxd, Q * p.xyd);
                aw[5] = vfma(P, p.y, -(Q * p.x));
                aw[6] = -(w_c * p.bct);
            }
            if constexpr (VAR == 2)
                acc[0] += ((aw[0] + aw[1]) + (aw[2] + aw[3])) + ((aw[4] + aw[5]) + aw[6]);
            else
                accum_row(acc, aw);
            {
                const float W = w_d * p.twd, Pd = w_d * p.pd, Qd = w_d * p.qd;
                aw[0] = -Pd;
                aw[1] = -Qd;
                aw[2] = vfma(Pd, p.xd, vfma(Qd, p.yd, W));
                aw[3] = vfma(Pd, p.xyd, vfma(Qd, p.yyd, W * p.y));
                aw[4] = -vfma(Pd, p.xxd, vfma(Qd, p.xyd, W * p.x));
                aw[5] = vfma(Pd, p.y, -(Qd * p.x));
                aw[6] = -(w_d * p.bdt);
            }
            if constexpr (VAR == 2)
                acc[0] += ((aw[0] + aw[1]) + (aw[2] + aw[3])) + ((aw[4] + aw[5]) + aw[6]);
            else
                accum_row(acc, aw);
        }
        rv = nx;
        if constexpr (VAR == 0) {
            if (++since == SF_P1_FLUSH) {  // uniform: every lane of the wave has made the same number of trips
                since = 0;
                p1_flush(acc, s, k.set, k.leader);
            }
        }
    }
}

template <int VAR>
__device__ __noinline__ void irls_pass1(const KArgs &a, int b, int L, int window_px, LDS SolveShared &s, int tid) {
    const IrlsCtx c = make_irls_ctx(a, b, L, s);
    const int lane = tid & 63, wave = tid >> 6;
    P1Consts k;
    k.inv_c_Cauchy = 1.f / (a.p.kc_Cauchy * uniform_f(s.aver_res));
#if SF_P1_FOLD
    k.fold_kc = c.g.inv_max_c * c.g.kph, k.fold_kd = c.g.inv_max_d;                              // pre-weight = k rsq(a)
    k.fold_gc = k.fold_kc * k.inv_c_Cauchy, k.fold_gd = k.fold_kd * k.inv_c_Cauchy;
#endif
    float acc[27];
#pragma unroll
    for (int q = 0; q < 27; q++) acc[q] = 0.f;
    k.set = tid / P1_GROUP;
    k.leader = (tid % P1_GROUP) == 0;
    if (lane < P1_SETS_PER_WAVE) {  // this wave's sets (nobody else touches them: no barrier, LDS operations of a wave are ordered)
#pragma unroll
        for (int q = 0; q < 27; q++) s.p1[q][wave * P1_SETS_PER_WAVE + lane] = 0.0;
    }
#pragma unroll
    for (int q = 0; q < 6; q++) k.Vr[q] = uniform_f(s.Var[q]);
    k.last = (c.n - 2) & ~1;  // the prefetch past the end re-reads the last pair instead of branching
    bool nt_first;
    int nt_next;
    pass_division(c.begin, c.n, window_px, nt_first, nt_next);
    RecVec<2> rv;
    // the trip count is the WAVE's (its first lane's): every lane stays active to the end, so that the group sums of a
    // flush see all their lanes; a lane past the end re-reads the last pair with weight 0
    load_first_rec(c.rp, min(c.begin + tid * 2, k.last), nt_first, rv);
    __builtin_amdgcn_s_waitcnt(SF_WAIT_VMCNT0);
    int since = 0;  // (the flush cadence runs through both loop instances)
    int i0 = c.begin + tid * 2, iw = uniform_i(c.begin + (tid - lane) * 2);
    p1_trips<VAR, true>(c, s, k, min(c.n, iw + nt_next * (SF_NT * 2)), i0, iw, rv, acc, since);
    p1_trips<VAR, false>(c, s, k, c.n, i0, iw, rv, acc, since);
    p1_flush(acc, s, k.set, k.leader);
    // this wave's sets, in order -> s.red[wave][0..26]
    __builtin_amdgcn_wave_barrier();
    if (lane < 27) {
        double t = 0.0;
#pragma unroll
        for (int g = 0; g < P1_SETS_PER_WAVE; g++) t += s.p1[lane][wave * P1_SETS_PER_WAVE + g];
        s.red[wave][lane] = t;
    }
}

// all threads: the 27 sums of pass 1 over the waves of this workgroup, then over the workgroups of the cluster (fixed
// orders: every workgroup ends up with the same bits) -> s.red[0][0..26]
__device__ __forceinline__ void irls_reduce_normal(LDS SolveShared &s, LDS ClusterShared &cs, int tid) {
    if (tid < 27) {
        double t = 0.0;
        for (int w = 0; w < SF_NW; w++) t += s.red[w][tid];
        put_f64(&cs.in[2 * tid], t);
    }
    cluster_gather(cs, 54, tid);
    if (tid < 27) {
        const int G = cl_G(cs);
        double t = 0.0;
        for (int p = 0; p < G; p++) t += get_f64(&cs.all[p * 54 + 2 * tid]);
        s.red[0][tid] = t;
    }
    __syncthreads();
}

// wave 0: AtA / AtB from the reduced sums, Var = AtA.ldlt().solve(AtB) (reference :640-642)
__device__ __noinline__ void irls_solve_normal(LDS SolveShared &s, int lane) {
    if (lane < 36) {
        const int i = lane / 6, j = lane - 6 * i;
        const int lo = min(i, j), hi = max(i, j);
        const int q = lo * 6 - (lo * (lo - 1)) / 2 + (hi - lo);  // upper-triangular packing of pass 1
        const float v = (float)s.red[0][q];
        s.AtA[lane] = v;
        s.M6[i * 7 + j] = v;
    }
    if (lane < 6) {
        const float v = (float)s.red[0][21 + lane];
        s.AtB[lane] = v;
        s.y6[lane] = v;
    }
    __builtin_amdgcn_wave_barrier();
    const bool az = ldlt_factor_wave<6>(s.M6, s.tmp6, s.tr6, lane);
    ldlt_solve_wave<6>(s.M6, s.tr6, az, s.y6, lane);
    if (lane < 6) s.Var[lane] = s.y6[lane];
    if (lane < SF_NC) s.lab_sum[lane] = 0;
}

// all threads, after pass 2: the per-label sums (exact integers) and ||res||^2 over the workgroups of the cluster
__device__ __forceinline__ void irls_reduce_residuals(LDS SolveShared &s, LDS ClusterShared &cs, int tid) {
    if (tid < SF_NC) put_i64(&cs.in[2 * tid], s.lab_sum[tid]);
    if (tid == SF_NC) {
        double q = 0.0;
        for (int w = 0; w < SF_NW; w++) q += s.red[w][27];
        put_f64(&cs.in[2 * SF_NC], q);
    }
    cluster_gather(cs, 2 * SF_NC + 2, tid);
    const int G = cl_G(cs);
    if (tid < SF_NC) {
        long long t = 0;
        for (int p = 0; p < G; p++) t += get_i64(&cs.all[p * (2 * SF_NC + 2) + 2 * tid]);
        s.lab_sum[tid] = t;
    }
    if (tid == SF_NC) {
        double q = 0.0;
        for (int p = 0; p < G; p++) q += get_f64(&cs.all[p * (2 * SF_NC + 2) + 2 * SF_NC]);
        s.sq_total = q;
    }
    __syncthreads();
}

// non-negative float (< 2^20) -> Q32.32 fixed point without the emulated float->int64 conversion
__device__ __forceinline__ unsigned long long to_fix32_pos(float x) {
    float y = x;
    if (!(y < 1.0e6f)) y = 1.0e6f;  // also catches NaN
    const unsigned hi = (unsigned)y;              // floor
    const float frac = y - (float)hi;              // exact
    const unsigned lo = (unsigned)(frac * 4294967296.f);
    return ((unsigned long long)hi << 32) | lo;
}

// pass 2: residuals with the new solution, per-label sums, ||res||^2 (reference :644-667).
// Per-label sums: each lane keeps a running fixed-point sum for the label of its last pixel and
// flushes it to the workgroup bins (LDS integer atomics: order-independent) only when the label
// changes -- labels are spatially coherent, so flushes are rare.
// DIR: 0 walks the pairs of [begin, n) upwards, as pass 1 does; 1 walks the SAME pairs from the top down (the first trip covers
// the last SF_NT pairs, i0 falls by SF_NT * 2 per trip, lanes keep ascending addresses inside a trip), so that the pass starts
// on the records pass 1 has just read and ends at `begin`, where the next pass 1 starts. The per-label
// sums are integers: the same bits in either direction; sq changes the order of its fp64 sum only.
// the trips of pass 2 from i0 until it passes `stop` (DIR 0: i0 < stop; DIR 1: i0 >= stop); NT: the policy of the record each trip
// loads (the next one's)
template <int VAR, int DIR, bool NT>
__device__ __forceinline__ void p2_trips(const IrlsCtx &c, LDS SolveShared &s, const float (&Vr)[6], int last, int stop, int &i0, RecVec<2> &rv,
                                         double &sq, int &cur_lab, unsigned long long &cur_sum) {
    const int step = DIR ? -SF_NT * 2 : SF_NT * 2;
    RecVec<2> nx;
    for (; DIR ? i0 >= stop : i0 < stop; i0 += step) {
        load_rec<2, NT>(c.rp, DIR ? max(i0 + step, c.begin) : min(i0 + step, last), nx);  // next pair in flight during this one
        const bool ok0 = sanitize<2>(rv, 0), ok1 = sanitize<2>(rv, 1);
        if constexpr (VAR == 1) {
            float t = rv.dn[0] + rv.dn[1];
#pragma unroll
            for (int q = 0; q < R_COUNT; q++) t += rv.v[q][0] + rv.v[q][1];
            sq += (double)t;
            rv = nx;
            continue;
        }
        float fu0, fv0;
        split_index(c.g, i0, fu0, fv0);
#pragma unroll
        for (int px = 0; px < 2; px++) {
            const bool ok = px ? ok1 : ok0;
            float fu = fu0, fv = fv0;
            if (px) {
                const bool wrap = (fv0 + 1.f) >= (float)c.g.rows_i;
                fu = wrap ? fu0 + 1.f : fu0;
                fv = wrap ? 0.f : fv0 + 1.f;
            }
            PixFact<float> p;
            fact_from_record<float>(c.g, fu, fv, rv.dn[px], rv.v[R_DW][px], rv.v[R_DCU][px], rv.v[R_DCV][px], rv.v[R_DCT][px],
                                    rv.v[R_DDU][px], rv.v[R_DDV][px], p);
            float rc, rd;
            fact_residuals<float>(p, Vr, rc, rd);
            const float rcs = ok ? rc : 0.f;
            const float rds = ok ? rd : 0.f;
            sq = fma((double)rcs, (double)rcs, sq);
            sq = fma((double)rds, (double)rds, sq);
            const unsigned long long fx = to_fix32_pos(fabsf(rcs) + fabsf(rds));
            if constexpr (VAR == 2) {
                sq += (double)(unsigned)(fx >> 32);
                continue;
            }
            const int lab = ok ? rv.lab[px] : cur_lab;
            if (lab != cur_lab) {
                if (cur_sum) lds_add(&s.lab_sum[cur_lab], (long long)cur_sum);
                cur_lab = lab;
                cur_sum = 0;
            }
            cur_sum += fx;
        }
        rv = nx;
    }
}

template <int VAR, int DIR = 0>
__device__ __noinline__ void irls_pass2(const KArgs &a, int b, int L, int window_px, LDS SolveShared &s, int tid) {
    const IrlsCtx c = make_irls_ctx(a, b, L, s);
    const int lane = tid & 63, wave = tid >> 6;
    float Vr[6];
#pragma unroll
    for (int q = 0; q < 6; q++) Vr[q] = uniform_f(s.Var[q]);
    double sq = 0.0;
    int cur_lab = 0;
    unsigned long long cur_sum = 0;
    const int last = (c.n - 2) & ~1;
    // DIR 1: the pair of lane 0 in the first trip lies SF_NT pairs below the end of the range (below `begin` in a range of fewer
    // pairs: those lanes make no trip); begin is even, so every pair starts where a pair of the upward walk starts
    const int step = DIR ? -SF_NT * 2 : SF_NT * 2;
    const int start = (DIR ? c.begin + ((c.n - c.begin + 1) & ~1) - SF_NT * 2 : c.begin) + tid * 2;
    // the window is where the sweep ENDS: the top of the range for the upward walk, [begin, begin + window) for the walk back down
    bool nt_first;
    int nt_next;
    pass_division(c.begin, c.n, window_px, nt_first, nt_next);
    RecVec<2> rv;
    if (DIR ? start >= c.begin : start < c.n) load_first_rec(c.rp, start, nt_first, rv);
    __builtin_amdgcn_s_waitcnt(SF_WAIT_VMCNT0);
    int i0 = start;
    p2_trips<VAR, DIR, true>(c, s, Vr, last, DIR ? max(c.begin, start + nt_next * step + 1) : min(c.n, start + nt_next * step), i0, rv, sq, cur_lab,
                             cur_sum);
    p2_trips<VAR, DIR, false>(c, s, Vr, last, DIR ? c.begin : c.n, i0, rv, sq, cur_lab, cur_sum);
    if (cur_sum) lds_add(&s.lab_sum[cur_lab], (long long)cur_sum);
    sq = wave_sum_f64(sq);
    if (lane == 0) s.red[wave][27] = sq;
}

#include "sf_reforder_solver.h"  // (empty unless SF_REFORDER; it needs what stands above)

// wave 0: build and factorise A_seg^T A_seg once per outer iteration
// (reference SegmentationBackground.cpp:105-130,143-165)
__device__ __noinline__ void irls_seg_factor(const KArgs &a, LDS SolveShared &s, int lane) {
    const float lambda_prior = a.p.lambda_prior;
    const float weight_reg = 2.f * a.p.lambda_reg;
    const float w2 = weight_reg * weight_reg, nw2 = weight_reg * (-weight_reg);
    if (lane < SF_NC) {
        const int l = lane;
        const float lt = s.lambda_t_w[l];
        const float dg = (lt > 0.1f) ? 2.f * lt * lambda_prior : 2.f * lt;
        s.seg_diag[l] = dg;
        const unsigned cm = s.conn[l];
        double dd = (double)(dg * dg);
        for (int lc = 0; lc < SF_NC; lc++) {
            const bool con = (lc != l) && ((cm >> lc) & 1u);
            if (con) dd += (double)w2;
            if (lc != l) s.M24[l * (SF_NC + 1) + lc] = con ? nw2 : 0.f;
        }
        s.M24[l * (SF_NC + 1) + l] = (float)dd;
    }
    __builtin_amdgcn_wave_barrier();
    const bool az = ldlt_factor_wave<SF_NC>(s.M24, s.tmp24, s.tr24, lane);
    if (lane == 0) s.seg_allzero = az ? 1 : 0;
}

// wave 0, after pass 2: averages, solveSegmIteration, convergence test (reference :666-683)
__device__ __noinline__ void irls_iteration_tail(const KArgs &a, LDS SolveShared &s, int N, int k, int lane) {
    const bool seg = a.p.segmentation_enabled != 0;
#if !SF_REFORDER  // (the reference-order build's pass 2 leaves the sequential float sums there itself)
    if (lane < SF_NC) s.aver_res_label[lane] = (float)((double)s.lab_sum[lane] * (1.0 / 4294967296.0));
#endif
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) {
        double t = 0.0;
        for (int l = 0; l < SF_NC; l++) t += (double)s.aver_res_label[l];
        s.aver_res_old = s.aver_res;
        s.aver_res = (float)t / float(2 * N);
        s.res_sqnorm = (float)s.sq_total;
    }
    __builtin_amdgcn_wave_barrier();
    if (seg) {
        // solveSegmIteration (reference SegmentationBackground.cpp:133-174)
        if (lane < SF_NC) {
            const int l = lane;
            const int npl = s.valid_cnt[l] + 1;  // num_pix_label starts at 1 (reference :651)
            const float arl = s.aver_res_label[l] / float(2 * npl);
            const float aro = s.aver_res_old;  // the PREVIOUS iteration's overall average (reference :652,672)
            const float kc = a.p.kc_Cauchy;
            const float repr_res = std_max(0.001f, aro);
            const float fixed_term = (float)log((double)(1.f + sqf(s.kb * repr_res / (kc * aro))));
            const float mult_res = 1.f / (kc * aro);
            const float lt = s.lambda_t_w[l];
            float Bseg;
            if (lt > 0.1f) {
                const float dataterm = fixed_term - (float)log((double)(1.f + sqf(arl * mult_res)));
                Bseg = dataterm + 2.f * a.p.lambda_prior * lt * s.b_prior[l];
            } else {
                Bseg = 2.f * lt * s.b_prior[l];
            }
            s.y24[l] = s.seg_diag[l] * Bseg;
        }
        __builtin_amdgcn_wave_barrier();
        ldlt_solve_wave<SF_NC>(s.M24, s.tr24, s.seg_allzero != 0, s.y24, lane);
        if (lane < SF_NC) s.b_segm[lane] = std_max(-1.f, std_min(2.f, s.y24[lane]));
    }
    if (lane == 0) {
        float delta = 0.f;
        for (int c = 0; c < 6; c++) delta = std_max(delta, fabsf(s.prev_sol[c] - s.Var[c]));
        for (int c = 0; c < 6; c++) s.prev_sol[c] = s.Var[c];
        s.last_delta = delta;
        s.ctrl = ((delta < a.p.irls_delta_threshold) || (k == a.p.max_iter_irls)) ? 1 : 0;
        s.n_irls++;
        s.pixel_iters += N;
    }
}

__device__ __noinline__ void solve_irls(const KArgs &a, int b, int L, int level, int kouter, bool forward, int window_px, LDS SolveShared &s, LDS ClusterShared &cs, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    const bool seg = a.p.segmentation_enabled != 0;
    const int N = __builtin_amdgcn_readfirstlane(s.n_valid);
    const int n_outer_now = __builtin_amdgcn_readfirstlane(s.n_outer);
    // the trace is written by ONE workgroup of a cluster (all of them hold the same values)
    sf_outer_trace *tr = (n_outer_now < SF_MAX_OUTER && cl_writer(cs)) ? &a.stats[b].outer[n_outer_now] : nullptr;

    // b initialisation (reference :603-607)
    if (tid < SF_NC) {
        if (!seg)
            s.b_segm[tid] = 1.f;
        else if (level == 0)
            s.b_segm[tid] = s.b_prior[tid];
    }
    if (tid < 6) {
        s.Var[tid] = 0.f;
        s.prev_sol[tid] = 0.f;
    }
    if (tid == 0) {
        int pb, pe;
        cluster_range(cs, a.ln[L], 2, pb, pe);  // the passes walk pixel pairs
        s.px_begin = pb;
        s.px_end = pe;
        s.rec_slot = cs.slot;
    }
    __syncthreads();

    if (N == 0) {  // defined behaviour for an empty level: nothing moves
        if (tid < 6) s.twist_level[tid] = 0.f;
        if (tr) {
            if (tid == 0) {
                tr->level = level; tr->k = kouter; tr->n_valid = 0; tr->irls_iters = 0; tr->aver_res = 0.f;
                tr->delta_sol_max = 0.f;
            }
            if (tid < 6) tr->var[tid] = tr->twist_level[tid] = tr->AtB[tid] = 0.f;
            if (tid < 16) tr->T[tid] = s.T[tid];
            if (tid < 36) tr->AtA[tid] = 0.f;
            if (tid < SF_NC) {
                tr->b_segm[tid] = s.b_segm[tid];
                tr->b_prior[tid] = s.b_prior[tid];
                tr->lambda_t_w[tid] = s.lambda_t_w[tid];
            }
        }
        __syncthreads();
        return;
    }

    // initial aver_res = mean |res| with res = -B (reference :588-590). B = (pre-weight / max) * derivative:
    // the sums of raw pre-weight x |dct|, |ddt| come from the linearisation, so no extra pass over the records
#if SF_REFORDER
    ro_initial_residual(a, b, L, s, tid);  // from the rows' B, as the reference does
#else
    if (tid == 0) {
        const double t = (double)(s.inv_max_c * a.p.k_photometric_res) * s.init_abs_c + (double)s.inv_max_d * s.init_abs_d;
        s.aver_res = (float)t / float(2 * N);
    }
#endif
    if (seg && wave == 0) irls_seg_factor(a, s, lane);
    __syncthreads();
    PROF_MARK(s, tid, PF_IRLS_INIT);

    int iters_done = 0;
    for (int k = 1; k <= a.p.max_iter_irls; k++) {
        iters_done = k;
#if SF_REFORDER
        ro_pass1(a, b, L, s, tid);
#else
        irls_pass1<0>(a, b, L, window_px, s, tid);
#endif
        __syncthreads();
        irls_reduce_normal(s, cs, tid);
        PROF_MARK(s, tid, PF_PASS1);
        if (wave == 0) irls_solve_normal(s, lane);
        __syncthreads();
        PROF_MARK(s, tid, PF_SOLVE6);
#if SF_REFORDER
        ro_pass2(a, b, L, s, tid);
#else
        // serpentine: pass 1 ends at the top of the records, pass 2 starts there and ends where the next pass 1 starts, so each
        // pass begins on the lines its predecessor touched last (uniform branch; `forward` is the old order, for tests and A/B).
        // window_px (uniform, from the launch): only that many pixels at the end of each sweep are loaded to stay cached (pass_division)
        if (forward)
            irls_pass2<0, 0>(a, b, L, window_px, s, tid);
        else
            irls_pass2<0, 1>(a, b, L, window_px, s, tid);
#endif
        __syncthreads();
        irls_reduce_residuals(s, cs, tid);
        PROF_MARK(s, tid, PF_PASS2);
        if (wave == 0) irls_iteration_tail(a, s, N, k, lane);
        __syncthreads();
        PROF_MARK(s, tid, PF_TAIL);
        if (__builtin_amdgcn_readfirstlane(s.ctrl)) break;
    }

    if (tr && wave == SF_NW - 1) {  // the trace: a wave that is not busy with the filter (one wave: after it, in order)
        if (lane == 0) {
            tr->level = level; tr->k = kouter; tr->n_valid = N; tr->irls_iters = iters_done;
            tr->aver_res = s.aver_res;
            tr->delta_sol_max = s.last_delta;
        }
        if (lane < 6) {
            tr->var[lane] = s.Var[lane];
            tr->AtB[lane] = s.AtB[lane];
        }
        if (lane < 36) tr->AtA[lane] = s.AtA[lane];
        if (lane < SF_NC) {
            tr->b_prior[lane] = s.b_prior[lane];
            tr->lambda_t_w[lane] = s.lambda_t_w[lane];
        }
    }
    if (wave == 0) solve_filter_and_update(a, s, level, lane);
    __syncthreads();
    if (tr) {
        if (tid < 6) tr->twist_level[tid] = s.twist_level[tid];
        if (tid < SF_NC) tr->b_segm[tid] = s.b_segm[tid];
        if (tid < 16) tr->T[tid] = s.T[tid];
    }
    __syncthreads();
    PROF_MARK(s, tid, PF_FILTER);
}
