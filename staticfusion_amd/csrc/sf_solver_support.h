// sf_solver_support.h — test and measurement support of the solver; never part of a solve.
#pragma once

#include "sf_irls.h"

// ---------------------------------------------------------------------------------------------
//  test support (sf_get_jacobian_rows): the rows of A and B of the LAST outer iteration of stream b, expanded
//  from the factored per-pixel form the passes evaluate: a_c = pc g1 + qc g2, a_d = twd g3 + pd g1 + qd g2,
//  b_c = -bct, b_d = -bdt (sf_irls.h). out = 14 planes of n pixels: a_c[0..5], b_c, a_d[0..5], b_d; pixels outside
//  validPixels get NaN in plane 0. Never part of a solve.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void debug_rows(const KArgs &a, int b, float *out, int gtid, int gstride) {
    const StreamState &st = a.state[b];
    const int L = st.last_level;
    const int n = a.ln[L], rows_i = a.lrows[L], cols_i = a.lcols[L];
    const size_t rb = (size_t)st.last_slot * a.n0;
    const float f = float(cols_i) / (2.f * a.tan_half_fovh);
    LevelGeom g;
    g.rows_i = rows_i;
    g.inv_rows = 1.f / float(rows_i);
    g.disp_u_i = 0.5f * float(cols_i - 1);
    g.disp_v_i = 0.5f * float(rows_i - 1);
    g.inv_f_pyr = 2.f * a.tan_half_fovh / float(cols_i);
    g.inv_f_w = 1.f / f;
    g.f_inv = f;
    g.kph = a.p.k_photometric_res;
    g.inv_max_c = st.inv_max_c;
    g.inv_max_d = st.inv_max_d;
    g.first = st.last_first;
    const float *dnew = pyr_level(a, b, 0, 0, L);
    for (int idx = gtid; idx < n; idx += gstride) {
        const float dw = a.rec[R_DW][rb + idx];
#if SF_REFORDER
        const bool in_valid = a.rec_lab[rb + idx] != SF_INVALID_LABEL;  // (this build's records keep the warp's own sign)
#else
        const bool in_valid = dw > 0.f;
#endif
        if (!in_valid) {
            out[idx] = __int_as_float(0x7fc00000);
            continue;
        }
        float fu, fv;
        split_index(g, idx, fu, fv);
        PixFact<float> p;
        fact_from_record<float>(g, fu, fv, dnew[idx], dw, a.rec[R_DCU][rb + idx], a.rec[R_DCV][rb + idx], a.rec[R_DCT][rb + idx],
                                a.rec[R_DDU][rb + idx], a.rec[R_DDV][rb + idx], p);
        const float g1[6] = {-1.f, 0.f, p.xd, p.xyd, -p.xxd, p.y};
        const float g2[6] = {0.f, -1.f, p.yd, p.yyd, -p.xyd, -p.x};
        const float g3[6] = {0.f, 0.f, 1.f, p.y, -p.x, 0.f};
        for (int c = 0; c < 6; c++) {
            out[(size_t)c * n + idx] = vfma(p.pc, g1[c], p.qc * g2[c]);
            out[(size_t)(7 + c) * n + idx] = vfma(p.twd, g3[c], vfma(p.pd, g1[c], p.qd * g2[c]));
        }
        out[(size_t)6 * n + idx] = -p.bct;
        out[(size_t)13 * n + idx] = -p.bdt;
    }
}

// ---------------------------------------------------------------------------------------------
//  measurement support: the two IRLS streaming passes in isolation, over the level-0 records the
//  last solve left behind (tools/pass_microbench.py, sf_microbench_pass)
//  WHICH 1 / 2: that pass alone. WHICH 3 / 4: one IRLS iteration's traffic, pass 1 then pass 2 back to back over the same
//  range, pass 2 upwards (3) or back down (4: the serpentine order of solve_irls). L > 0 walks the first ln[L] pixels of the
//  same record planes with that level's geometry and depth plane: the values mean nothing there, the bytes and the
//  instructions are the level's (sanitize() keeps every row finite). window_px: the load policy of the sweeps, as in a solve.
// ---------------------------------------------------------------------------------------------
template <int WHICH, int VAR>
__device__ void microbench_pass(const KArgs &a, int b, int L, int slice, int slices, int reps, int window_px, LDS SolveShared &s, int tid) {
    const StreamState &st = a.state[b];
    if (tid < SF_NC) s.b_segm[tid] = a.p.segmentation_enabled ? st.b_segm[tid] : 1.f;
    if (tid < 6) s.Var[tid] = st.twist_level[tid];
    if (tid == 0) {
        s.inv_max_c = st.inv_max_c;
        s.inv_max_d = st.inv_max_d;
        s.rec_slot = b;
        s.aver_res = 0.002f;
        s.first = 0;
        s.n_valid = a.ln[L];
        const int per = ((a.ln[L] / slices) + 1) & ~1;  // even: the passes walk pixel pairs
        s.px_begin = slice * per;
        s.px_end = (slice == slices - 1) ? a.ln[L] : min(a.ln[L], (slice + 1) * per);
    }
    if (tid < SF_NC) s.lab_sum[tid] = 0;
    __syncthreads();
    for (int r = 0; r < reps; r++) {
        if (WHICH != 2) {
            irls_pass1<VAR>(a, b, L, window_px, s, tid);
            __syncthreads();
        }
        if (WHICH != 1) {
            irls_pass2<VAR, WHICH == 4>(a, b, L, window_px, s, tid);
            __syncthreads();
        }
    }
}

