// sf_warp.h — the warp stage of the solve (solve_warp); sf_solver.h has the map of the stage headers.
#pragma once

#include "sf_cluster.h"
#include "sf_reforder.h"  // splat_ordered, ordered_splat, ro_list_of
#include "sf_smallmath.h"
#include "sf_solve_shared.h"
#include "sf_splat.h"

// ---------------------------------------------------------------------------------------------
//  warp (reference FrontEnd.cpp:775-892), scatter part.  Normalisation happens when the
//  accumulators are read by the linearisation.
// ---------------------------------------------------------------------------------------------
__device__ __noinline__ void solve_warp(const KArgs &a, int b, int L, LDS SolveShared &s, LDS ClusterShared &cs, int tid) {
    const int rows_i = a.lrows[L], cols_i = a.lcols[L], n = a.ln[L];
    const int G = cl_G(cs), rank = cl_rank(cs);
    const size_t rb = (size_t)cl_slot(cs) * a.n0;
    const auto dpred = as_global(pyr_level(a, b, 1, 0, L)), ipred = as_global(pyr_level(a, b, 1, 1, L));
    const auto acc_d = as_global(a.acc_d + rb);
    const auto acc_i = as_global(a.acc_i + rb);

    if (tid == 0) inverse4_cm(s.T, s.Tinv, s.dwork);  // T = T_odometry.inverse()  (:800)
    // a cluster's workgroups zero every G-th block. Agent-scope (write-through) stores: the cells are only ever touched by
    // agent-scope atomics and atomic loads after this, so the two hand-overs below need no fence (sf_cluster.h)
    // coarse levels (and every level of the reference-order build): the reference's float sums in the reference's order
    // (uniform by construction, made so for the compiler: branches around barriers must be scalar branches, see ordered_splat)
    const bool ordered = uniform_i(splat_ordered(n, G) ? 1 : 0) != 0;
    const bool lazy = ordered || uniform_i(splat_lazy_ok(rows_i, cols_i, G) ? 1 : 0) != 0;  // one workgroup: the splat zeroes / initialises the cells itself
    if (!lazy)
    for (int idx = tid + rank * SF_NT; idx < n; idx += SF_NT * G) {
        if (G > 1) {
            __hip_atomic_store(acc_d + idx, 0ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(acc_i + idx, 0ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            gst(acc_d, idx, 0ll);
            gst(acc_i, idx, 0ll);
        }
    }
    cluster_rendezvous(cs, tid);  // the accumulators are zero everywhere before anybody splats into them (and s.Tinv is set)

    SplatGeom g;
    g.f = float(cols_i) / (2.f * a.tan_half_fovh);
    g.disp_u_i = 0.5f * float(cols_i - 1);
    g.disp_v_i = 0.5f * float(rows_i - 1);
    g.cols_lim = 100 * (cols_i - 1);
    g.rows_lim = 100 * (rows_i - 1);
    g.rows_i = rows_i;
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) g.T[r * 4 + c] = uniform_f(s.Tinv[r + 4 * c]);

    struct Src {
        gptr<const float> d, i;
        LevelCoord lc;
        __device__ __forceinline__ bool load(int v, int u, int idx, float &z, float &xr, float &yr, float &iw) const {
            z = gld(d, idx);
            iw = gld(i, idx);
            xr = coord_x(lc, u, z);  // xxPrediction / yyPrediction of the pyramid (:385-386)
            yr = coord_y(lc, v, z);
            return z != 0.f;
        }
    } src{dpred, ipred, level_coord(a, L)};
    if (ordered)
        ordered_splat(a, g, level_coord(a, L), rows_i, cols_i, src, acc_d, acc_i, ro_list_of(a, rb, b), s.win, tid, &a.state[b].prof[PF_ORDERED_FALLBACKS]);
    else
        tiled_splat(g, rows_i, cols_i, src, acc_d, acc_i, s.win, s.marks, tid, rank, G, lazy, &a.state[b].prof[PF_SPLAT_REPLAYS]);
    cluster_rendezvous(cs, tid);  // all atomics of the workgroup(s) performed: the linearisation reads the cells with atomic loads
}
