// sf_p2p_system.h — the quantised point-to-plane SYSTEM, stated once for the three solvers that sum it: the pose refinement
// (sf_align.h), the region motions (sf_bodies.h) and the map registration (sf_register_rules.h). A pair with the row J = (Q x n, n)
// and the residual r = n . (Q - M) enters as the integers a = rint(clamp(J, +-64) * 2^12) and rho = rint(r * 2^16); a system is
// 32 int64 words: n, ss = sum rho^2, g[6] = sum a rho, H[21] = sum a a^T (k <= l, row-wise) and three reserved words written as 0
// (sfa_system, sfb_system and sfg_system of include/). The step that solves it: sf_align_step.h. Plain C++, fp32 in the written
// order, one operation per expression (no contraction: -ffp-contract=off), so the host, the device and tests/cpp/ run the same
// text and give the same bits. The cross product stays with each caller: the three spell it as their references do. It includes
// nothing of the library and defines no kernel.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define P2P_HD __host__ __device__
#else
#define P2P_HD
#endif

namespace p2p {

enum { FIELDS = 29, WORDS = 32 };               // the summed words of a system, and its words
enum { OK = 0, FEW_PAIRS = 1, DEGENERATE = 2 };  // how an entry ends: SFA_*, SFB_* and SFG_* of include/
constexpr float CLAMP = 64.0f, ROW_SCALE = 4096.0f, RES_SCALE = 65536.0f;

// |a| <= 2^18, and |rho| <= 2^16 for |r| <= 1 (dist_max <= 1). A NaN in J quantises to -CLAMP * ROW_SCALE: fmaxf returns the bound.
P2P_HD static inline void quantise(const float J[6], float r, int a[6], int *rho) {
    for (int k = 0; k < 6; k++) {
        const float lo = fmaxf(J[k], -CLAMP);
        const float cl = fminf(lo, CLAMP);
        a[k] = (int)rintf(cl * ROW_SCALE);
    }
    *rho = (int)rintf(r * RES_SCALE);
}

// the 29 sums take one pair (products of 32-bit factors)
P2P_HD static inline void accumulate(long long *acc, const int a[6], int rho) {
    acc[0] += 1;
    acc[1] += (long long)rho * rho;
    int f = 8;
    for (int k = 0; k < 6; k++) {
        acc[2 + k] += (long long)a[k] * rho;
        for (int l = k; l < 6; l++) acc[f++] += (long long)a[k] * a[l];
    }
}

}  // namespace p2p
