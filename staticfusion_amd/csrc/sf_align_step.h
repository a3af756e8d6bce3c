// sf_align_step.h — the STEP of include/sf_align.h: from the 32 int64 words of a system (sf_p2p_system.h) and the estimate D, the
// damped normal equations, their LDL^T solve without pivoting, the Cayley rotation of the solution and the updated estimate. fp64
// in the written order, only + - * / (no contraction: -ffp-contract=off), so the host (sfa_step of sf_hip_align.hip, and
// tests/cpp/align_step_host.cpp under the sanitizers) and the device (p2p_step_entry of sf_p2p_device.h) run the same text and
// give the same bits. It includes nothing of the library but sf_p2p_system.h and defines no kernel.
#pragma once
#include <stdint.h>

#include "sf_p2p_system.h"

#define SFA_HD P2P_HD
#define SFA_STEP_OK p2p::OK
#define SFA_STEP_DEGENERATE p2p::DEGENERATE
#define SFA_SYSTEM_WORDS p2p::WORDS

// w: the words of a sfa_system. Returns SFA_STEP_OK with D_out written (it may be D_in), or SFA_STEP_DEGENERATE with D_out
// untouched.
SFA_HD static inline int sfa_step_core(const int64_t *w, float damping, const double *D_in, double *D_out) {
    const double n = (double)w[0];
    double A[6][6], b[6], L[6][6] = {}, d[6] = {}, z[6] = {}, x[6] = {};
    int idx = 8;
    for (int k = 0; k < 6; k++)
        for (int l = k; l < 6; l++) {
            const double v = (double)w[idx++] * (1.0 / 16777216.0);  // 2^-24
            A[k][l] = v;
            A[l][k] = v;
        }
    const double lambda = (double)damping * n;
    for (int k = 0; k < 6; k++) {
        A[k][k] = A[k][k] + lambda;
        b[k] = -((double)w[2 + k] * (1.0 / 268435456.0));  // 2^-28
    }
    const double floor_d = 1e-9 * n;
    for (int j = 0; j < 6; j++) {
        double s = A[j][j];
        for (int k = 0; k < j; k++) s = s - (L[j][k] * L[j][k]) * d[k];
        if (!(s > floor_d)) return SFA_STEP_DEGENERATE;
        d[j] = s;
        for (int i = j + 1; i < 6; i++) {
            double t = A[i][j];
            for (int k = 0; k < j; k++) t = t - (L[i][k] * L[j][k]) * d[k];
            L[i][j] = t / s;
        }
    }
    for (int i = 0; i < 6; i++) {
        double t = b[i];
        for (int k = 0; k < i; k++) t = t - L[i][k] * z[k];
        z[i] = t;
    }
    for (int i = 5; i >= 0; i--) {
        double t = z[i] / d[i];
        for (int k = i + 1; k < 6; k++) t = t - L[k][i] * x[k];
        x[i] = t;
    }
    const double a0 = 0.5 * x[0], a1 = 0.5 * x[1], a2 = 0.5 * x[2];
    const double aa = (a0 * a0 + a1 * a1) + a2 * a2;
    const double s = 2.0 / (1.0 + aa);
    double R[3][3];
    R[0][0] = 1.0 - s * (a1 * a1 + a2 * a2);
    R[0][1] = s * (a0 * a1 - a2);
    R[0][2] = s * (a0 * a2 + a1);
    R[1][0] = s * (a0 * a1 + a2);
    R[1][1] = 1.0 - s * (a0 * a0 + a2 * a2);
    R[1][2] = s * (a1 * a2 - a0);
    R[2][0] = s * (a0 * a2 - a1);
    R[2][1] = s * (a1 * a2 + a0);
    R[2][2] = 1.0 - s * (a0 * a0 + a1 * a1);
    double out[12];
    for (int k = 0; k < 3; k++)
        for (int c = 0; c < 4; c++) {
            double v = (R[k][0] * D_in[c] + R[k][1] * D_in[4 + c]) + R[k][2] * D_in[8 + c];
            if (c == 3) v = v + x[3 + k];
            out[4 * k + c] = v;
        }
    for (int k = 0; k < 12; k++) D_out[k] = out[k];
    return SFA_STEP_OK;
}

// pose = T0 * D rounded to float, column-major (include/sf_align.h, LOOP)
SFA_HD static inline void sfa_compose_pose(const float *t0, const double *D, float *pose) {
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) {
            double v = ((double)t0[r] * D[c] + (double)t0[r + 4] * D[4 + c]) + (double)t0[r + 8] * D[8 + c];
            if (c == 3) v = v + (double)t0[r + 12];
            pose[r + 4 * c] = (float)v;
        }
}
