// sf_body_world.h — WORLD MOTION of include/sf_bodies.h: W = (T1 * D) * T0^-1 from two camera-to-world poses and the 3 x 4
// estimate D of a region, and D itself as a 4 x 4. fp64 in the written order, only + - * / (no contraction:
// -ffp-contract=off), T0^-1 formed by the transpose, every entry rounded to float once, so the host (sfb_world_motion of
// sf_hip_bodies.hip, and tests/cpp/body_world_host.cpp under the sanitizers) and the device (sfb_step_kernel of sf_bodies.h)
// run the same text and give the same bits. It includes nothing of the library and defines no kernel.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SFB_HD __host__ __device__
#else
#define SFB_HD
#endif

// pose0, pose1: column-major 4 x 4 (entry (r, c) at r + 4 c); D: row-major 3 x 4; w: column-major 4 x 4, 16 floats written
SFB_HD static inline void sfb_world_core(const float *pose0, const float *pose1, const double *D, float *w) {
    for (int r = 0; r < 3; r++) {
        double A[4], W[3];
        for (int c = 0; c < 4; c++) {
            const double x = (double)pose1[r] * D[c];
            const double y = (double)pose1[r + 4] * D[4 + c];
            const double z = (double)pose1[r + 8] * D[8 + c];
            const double xy = x + y;
            double v = xy + z;
            if (c == 3) v = v + (double)pose1[r + 12];
            A[c] = v;
        }
        for (int c = 0; c < 3; c++) {  // T0^-1 = (R0^T, -R0^T t0): column c of R0^T is row c of R0
            const double x = A[0] * (double)pose0[c];
            const double y = A[1] * (double)pose0[c + 4];
            const double z = A[2] * (double)pose0[c + 8];
            const double xy = x + y;
            W[c] = xy + z;
            w[r + 4 * c] = (float)W[c];
        }
        const double x = W[0] * (double)pose0[12];
        const double y = W[1] * (double)pose0[13];
        const double z = W[2] * (double)pose0[14];
        const double xy = x + y;
        const double back = xy + z;
        w[r + 12] = (float)(A[3] - back);
    }
    w[3] = 0.f;
    w[7] = 0.f;
    w[11] = 0.f;
    w[15] = 1.f;
}

// d[k + 4 c] = (float)D[k][c], last row 0 0 0 1
SFB_HD static inline void sfb_estimate_as_4x4(const double *D, float *d) {
    for (int k = 0; k < 3; k++)
        for (int c = 0; c < 4; c++) d[k + 4 * c] = (float)D[4 * k + c];
    d[3] = 0.f;
    d[7] = 0.f;
    d[11] = 0.f;
    d[15] = 1.f;
}
