// sf_motion_filter.h — covariance, eigen-space velocity filter and SE(3) update at the end of an outer iteration
// (solve_filter_and_update); sf_solver.h has the map of the stage headers.
#pragma once

#include "sf_smallmath.h"
#include "sf_solve_shared.h"

// ---------------------------------------------------------------------------------------------
//  filterEstimateAndComputeT (reference FrontEnd.cpp:713-772) + est_cov (:689). One lane.
// ---------------------------------------------------------------------------------------------
// Called by the whole wave 0: the 6 x 6 inverse and the Jacobi sweeps use six lanes (same arithmetic per element as
// one lane would do), everything else runs on lane 0.
__device__ __noinline__ void solve_filter_and_update(const KArgs &a, LDS SolveShared &s, int level, int lane) {
    // est_cov = AtA.inverse() * res.squaredNorm()
    LDS double *Ad = s.dwork, *V = s.dwork + 72;
    {
        double aa = (lane < 36) ? (double)s.AtA[lane] : 0.0, ainv;
        inverse6_lanes(aa, ainv, lane);
        if (lane < 36) s.est_cov[lane] = (float)ainv * s.res_sqnorm;
    }
    __builtin_amdgcn_wave_barrier();

    float twist[6];
    for (int i = 0; i < 6; i++) twist[i] = s.Var[i];

    if (a.p.use_motion_filter) {
        LDS double *S = Ad;  // reuse
        bool finite = true;
        for (int i = 0; i < 6; i++)  // uniform: every lane looks at the same 21 values
            for (int j = 0; j <= i; j++)
                if (!isfinite((double)s.est_cov[i * 6 + j])) finite = false;
        if (!finite) {  // "Eigensolver couldn't find a solution. Pose is not updated"
            if (lane == 0) s.status |= SF_STATUS_EIG_SKIPPED;
            return;
        }
        {
            const int l = (lane < 36) ? lane : 0, i = l / 6, j = l - 6 * i;
            double sa = (double)s.est_cov[(i >= j) ? i * 6 + j : j * 6 + i], vv;  // the lower triangle, mirrored
#if SF_REFORDER
            if (lane < 36) S[lane] = sa;
            __builtin_amdgcn_wave_barrier();
            jacobi_eig6_wave(S, V, lane);  // the cyclic order of the oracle ([C5]), element for element
            (void)vv;
#else
            jacobi6_lanes(sa, vv, lane);
            if (lane < 36) {
                S[lane] = sa;  // the diagonal holds the eigenvalues
                V[lane] = vv;
            }
#endif
        }
        __builtin_amdgcn_wave_barrier();
        if (lane != 0) return;
        float kai_loc_sub[6], lt[6];
        log_twist_cm(s.T, lt);
        for (int i = 0; i < 6; i++) kai_loc_sub[i] = s.twist_old[i] - lt[i];
        const float e_l = (float)exp(-(double)level);
        const float cf = a.p.previous_speed_eig_weight * e_l, df = a.p.previous_speed_const_weight * e_l;
        double kai_b_fil[6];
        for (int i = 0; i < 6; i++) {
            double kb_ = 0, kbo = 0;
            for (int r = 0; r < 6; r++) {
                kb_ += V[r * 6 + i] * (double)twist[r];
                kbo += V[r * 6 + i] * (double)kai_loc_sub[r];
            }
            const double wgt = (double)cf * S[i * 6 + i] + (double)df;
            kai_b_fil[i] = (kb_ + wgt * kbo) / (1.0 + wgt);
        }
        for (int r = 0; r < 6; r++) {
            double acc = 0;
            for (int i = 0; i < 6; i++) acc += V[r * 6 + i] * kai_b_fil[i];
            twist[r] = (float)acc;
        }
    }
    if (lane != 0) return;

    double xi[6], E[16];
    for (int i = 0; i < 6; i++) xi[i] = (double)twist[i];
    se3_exp_d(xi, E);
    float Ef[16], Tn[16];
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) Ef[r + 4 * c] = (float)E[r * 4 + c];
    for (int i = 0; i < 6; i++) s.twist_level[i] = twist[i];
    mul4_cm(Ef, s.T, Tn);
    for (int i = 0; i < 16; i++) s.T[i] = Tn[i];
    float tw[6];
    log_twist_cm(s.T, tw);
    for (int i = 0; i < 6; i++) s.twist[i] = tw[i];
}
