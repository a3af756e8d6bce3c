// sf_solver.h — the coarse-to-fine coupled odometry + segmentation solve of one stream.
// Replaces the loop of StaticFusion::runSolver (reference FrontEnd.cpp:1091-1144) and everything
// it calls: warpImagesAccurateInverse (:775-892), calculateCoord (:393-430), calculateDerivatives
// (:432-479), computeWeights (:481-510), computeSegPrior (SegmentationBackground.cpp:53-103),
// solveOdometryAndSegmJoint (:513-692) with buildSystemSegm / solveSegmIteration
// (SegmentationBackground.cpp:105-174) and filterEstimateAndComputeT (:713-772).
//
// Data flow per outer iteration at level L (N_L pixels):
//   warp        scatter the Pred level into 3 order-independent fixed-point accumulators
//               (64-bit integer atomics: the result does not depend on the scatter order)
//   linearise   register strips (a wave sweeps the columns of 62 rows; LDS tiles in the cluster build): Inter images,
//               edge-aware gradients, temporal differences, raw pre-weights  ->  11 float planes + 1 label byte per pixel
//               ("records", 45 B/px), plus the global max of the pre-weights and the per-label prior
//   IRLS        <= max_iter_irls iterations of two streaming passes over the records:
//                 pass 1  rebuild the two Jacobian rows, Cauchy x b weights, accumulate the 21+6
//                         normal-equation sums in fp64 registers -> wave shuffle -> LDS -> 6x6 LDL^T
//                 pass 2  residuals with the new solution, per-label |res| sums (fixed point),
//                         ||res||^2 -> 24x24 LDL^T for b, convergence test
//   filter      covariance, eigen-space velocity filter, SE(3) update (one lane, fp64)
// The Jacobian matrix A (2N x 6) of the reference is never materialised.
//
// One header per stage, included in this order (each includes what it uses):
//   sf_solve_shared.h   SolveShared (the workgroup's LDS state), tile / strip / pass-1 geometry, PROF_MARK
//   sf_warp.h           solve_warp            (the splat itself: sf_splat.h, sf_reforder.h)
//   sf_linearise.h      solve_linearise (cluster) / solve_linearise_strips, seg_prior_*, solve_seg_prior
//   sf_motion_filter.h  solve_filter_and_update
//   sf_irls.h           irls_pass1 / irls_pass2, reductions, small solves, solve_irls (records: sf_records.h)
//   here                stage_solve, the coarse-to-fine loop
// sf_solver_support.h (debug_rows, microbench_pass) is not part of a solve; the build axes are in sf_build_config.h.
#pragma once

#include "sf_cluster.h"
#include "sf_device_common.h"
#include "sf_smallmath.h"
#include "sf_solve_shared.h"
// (the stages in the order of the data flow, not of the alphabet: it is the order of their functions in the object)
#include "sf_warp.h"
#include "sf_linearise.h"
#include "sf_motion_filter.h"
#include "sf_irls.h"

// ---------------------------------------------------------------------------------------------
//  the coarse-to-fine loop (reference FrontEnd.cpp:1091-1144)
// ---------------------------------------------------------------------------------------------
// Levels of at most this many pixels are not worth a rendezvous per reduction: in the cluster build every workgroup runs
// them on its own (redundantly, on a private record slot) and all arrive at bit-identical state.
#define SF_CLUSTER_SOLO_PIXELS 8192

// forward (uniform, from the launch: ST_SOLVER_FORWARD): pass 2 of the IRLS walks upwards like pass 1 -- tests and A/B only
// window_px (uniform, FrameLaunch::pass_window_px): the pixels at the end of each IRLS sweep that are loaded to stay cached (sf_irls.h)
__device__ __noinline__ void stage_solve(const KArgs &a, int b, bool forward, int window_px, LDS SolveShared &s, LDS ClusterShared &cs, int tid) {
    StreamState &st = a.state[b];
    if (tid < 16) s.T[tid] = (tid % 5 == 0) ? 1.f : 0.f;  // T_odometry.setIdentity()  (:1091)
    if (tid < 6) {
        s.twist_old[tid] = st.twist_old[tid];
        s.twist[tid] = st.twist[tid];
        s.twist_level[tid] = st.twist_level[tid];
    }
    if (tid < SF_NC) {
        s.b_segm[tid] = st.b_segm[tid];
        s.conn[tid] = st.conn[tid];
        s.b_prior[tid] = st.b_prior[tid];
        s.lambda_t_w[tid] = st.lambda_t_w[tid];
    }
    if (tid < SF_PROF_SLOTS) s.prof[tid] = 0;
    if (tid == 0) {
        s.t_last = wall_clock64();
        s.kb = st.kb;
        s.status = 0;
        s.n_irls = 0;
        s.n_outer = 0;
        s.pixel_iters = 0;
    }
    __syncthreads();
    const bool clustered = uniform_i(cs.full_G) > 1;

    int last_L = 0;
    for (int i = 0; i < a.levels; i++) {
        const int L = a.levels - i - 1;  // image_level
        if (clustered) cluster_set_solo(cs, tid, a.ln[L] <= SF_CLUSTER_SOLO_PIXELS);
        for (int k = 0; k < a.p.max_iter_per_level; k++) {
            last_L = L;
            const bool first = (i == 0) && (k == 0);
            if (!first) solve_warp(a, b, L, s, cs, tid);
            PROF_MARK(s, tid, PF_WARP);
#if SF_LIN_STRIPS
            {
                const int which = (uniform_i(a.p.debug_planes) ? 4 : 0) | (first ? 2 : 0) | (uniform_i(a.p.segmentation_enabled) ? 1 : 0);
                switch (which) {  // (uniform)
                case 0: solve_linearise_strips<false, false, false>(a, b, L, s, cs, tid); break;
                case 1: solve_linearise_strips<false, false, true>(a, b, L, s, cs, tid); break;
                case 2: solve_linearise_strips<false, true, false>(a, b, L, s, cs, tid); break;
                case 3: solve_linearise_strips<false, true, true>(a, b, L, s, cs, tid); break;
                case 4: solve_linearise_strips<true, false, false>(a, b, L, s, cs, tid); break;
                case 5: solve_linearise_strips<true, false, true>(a, b, L, s, cs, tid); break;
                case 6: solve_linearise_strips<true, true, false>(a, b, L, s, cs, tid); break;
                default: solve_linearise_strips<true, true, true>(a, b, L, s, cs, tid); break;
                }
            }
#else
            solve_linearise(a, b, L, first, s, cs, tid);
#endif
#if SF_REFORDER
            if (a.p.segmentation_enabled) ro_seg_prior(a, b, L, s, cs, tid);
#else
#if SF_LIN_FUSED_PRIOR
            if (uniform_i(a.p.segmentation_enabled)) seg_prior_finish(s, cs, tid);  // (the sums: solve_linearise_strips)
#else
            if (a.p.segmentation_enabled) solve_seg_prior(a, b, L, s, cs, tid);
#endif
#endif
            PROF_MARK(s, tid, PF_LINEARISE);
            solve_irls(a, b, L, i, k, forward, window_px, s, cs, tid);
            if (tid == 0) {
                s.n_outer++;
                double s2 = 0.0;
#if SF_REFORDER  // the oracle's reading of twist_level_odometry.norm(): fp64 sum of the FLOAT squares
                for (int c = 0; c < 6; c++) s2 += (double)(s.twist_level[c] * s.twist_level[c]);
                const float nrm = (float)sqrt((double)(float)s2);
#else
                for (int c = 0; c < 6; c++) s2 += (double)s.twist_level[c] * (double)s.twist_level[c];
                const float nrm = sqrtf((float)s2);
#endif
                s.ctrl = (nrm < 0.04f) ? 1 : 0;  // reference :1130
            }
            __syncthreads();
            const int brk = __builtin_amdgcn_readfirstlane(s.ctrl);
            __syncthreads();
            if (brk) break;
        }
    }
    const int last_slot = cl_slot(cs);
    if (clustered) cluster_set_solo(cs, tid, false);

    // twist_odometry_old = R_inc^-1 * twist_odometry (reference :1139-1144)
    if (tid == 0) {
        LDS double *R = s.dwork, *Ri = s.dwork + 16;
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) R[r * 3 + c] = (double)s.T[r + 4 * c];
        inverse_double_lds(R, Ri, 3);
        float Rif[9];
        for (int q = 0; q < 9; q++) Rif[q] = (float)Ri[q];
        for (int half = 0; half < 2; half++)
            for (int r = 0; r < 3; r++) {
                float acc = Rif[r * 3 + 0] * s.twist[half * 3 + 0];
                acc += Rif[r * 3 + 1] * s.twist[half * 3 + 1];
                acc += Rif[r * 3 + 2] * s.twist[half * 3 + 2];
                s.twist_old[half * 3 + r] = acc;
            }
    }
    __syncthreads();
    const bool commit = commit_ok(cs);  // false: a rendezvous of this frame timed out somewhere in the cluster -- the values
                                        // in LDS may come from stale words; the stream keeps the state of its last good frame
    if (cl_writer(cs) && !commit && tid == 0) a.stats[b].status = s.status | SF_STATUS_SYNC_TIMEOUT;
    if (cl_writer(cs) && commit) {  // ONE workgroup of a cluster stores the stream's results (all of them hold the same values)
        if (tid == 0) {
            sf_frame_stats &fs = a.stats[b];
            fs.n_outer = s.n_outer;
            fs.n_irls = s.n_irls;
            fs.pixel_iters = s.pixel_iters;
            fs.status = s.status;
            st.last_level = last_L;
            st.last_first = s.first;
            st.last_slot = last_slot;
            st.cum_frames += 1;
            st.cum_irls += s.n_irls;
            st.cum_outer += s.n_outer;
            st.cum_pixel_iters += s.pixel_iters;
            st.inv_max_c = s.inv_max_c;
            st.inv_max_d = s.inv_max_d;
            if (!a.p.segmentation_enabled) fs.kmeans_iters = 0;
        }
        if (tid < 16) st.T[tid] = s.T[tid];
        if (tid < 6) {
            st.twist_old[tid] = s.twist_old[tid];
            st.twist[tid] = s.twist[tid];
            st.twist_level[tid] = s.twist_level[tid];
        }
        if (tid < 36) st.est_cov[tid] = s.est_cov[tid];
        if (tid >= PF_WARP && tid <= PF_FILTER) st.prof[tid] += s.prof[tid];
        if (tid < SF_NC) {
            st.b_segm[tid] = s.b_segm[tid];
            st.b_prior[tid] = s.b_prior[tid];
            st.lambda_t_w[tid] = s.lambda_t_w[tid];
        }
    }
    cluster_barrier(cs, tid);  // the stream state is visible to the stages that follow (in every workgroup)
}
