// sf_solve_shared.h — what the stages of the solve share: tile / strip / pass-1 geometry, the weight primitives, the
// workgroup's LDS state (SolveShared) and the in-kernel stage timer. sf_solver.h has the map of the stage headers.
#pragma once

#include "sf_device_common.h"
#include "sf_reforder.h"  // RoChunk, RoChunk2, RoRows (reference-order build)
#include "sf_splat.h"     // SplatWin, SplatMarks

#define LS_ROWS 62  // rows a wave owns in a strip (lanes 1 .. LS_ROWS; lane 0 and lane LS_ROWS + 1 hold the halo rows)
#define TILE_V 64
#define TILE_U (2 * SF_NT / TILE_V)  // two centre pixels per lane
#define TILE_LV (TILE_V + 2)
#define TILE_LU (TILE_U + 2)
#define TILE_N (TILE_LV * TILE_LU)

// Per-pixel IRLS weights use the hardware reciprocal / reciprocal-square-root (1 ulp) instead of the
// IEEE division + square root sequences (~10 VALU instructions each; pass 1 is VALU-bound). The
// linearisation (max weights, records) stays bit-identical to the oracle; the solver result moves by
// ~1e-7, three orders of magnitude inside the pose tolerance. -DSF_FAST_WEIGHTS=0 restores IEEE.
#if SF_FAST_WEIGHTS
__device__ __forceinline__ float vrsq(float x) { return __builtin_amdgcn_rsqf(x); }
__device__ __forceinline__ float vrcpw(float x) { return __builtin_amdgcn_rcpf(x); }
#else
__device__ __forceinline__ float vrsq(float x) { return sqrtf(1.f / x); }
__device__ __forceinline__ float vrcpw(float x) { return 1.f / x; }
#endif


struct LinTile {  // linearisation tile (with halo)
    float t_D[TILE_N], t_I[TILE_N];    // Inter depth / intensity
    float t_dn[TILE_N], t_in[TILE_N];  // new depth / intensity
    float t_dw[TILE_N], t_iw[TILE_N];  // warped depth / intensity
    uint8_t t_null[TILE_N];
};

// Pass 1 keeps the 27 normal-equation sums per lane in fp32 and, every SF_P1_FLUSH pixel pairs, adds them -- reduced over a
// group of P1_GROUP neighbouring lanes on the DPP network -- into fp64 sums in LDS (one set per lane group; entry-major, so
// the group leaders of a wave touch consecutive 8-byte words). A lane's fp32 partial sum then never holds more than
// 4 SF_P1_FLUSH terms: the rounding error of the accumulated AtA / AtB drops about tenfold against one fp32 sum over the
// lane's whole share (<= 600 terms at QVGA), which is what moved b by 4e-5 against the oracle's fp64 sums ([C1]).
#define SF_P1_FLUSH 32
#define P1_GROUP (SF_NT == 256 ? 4 : 16)  // 1024-thread builds: a lane sums a quarter of the terms, rows of 16 lanes share a set
#define P1_SETS (SF_NT / P1_GROUP)
#define P1_SETS_PER_WAVE (64 / P1_GROUP)

struct SolveShared {
    union {            // the warp window and the linearisation tile are never live together; the fp64 scratch of the
        LinTile lt;    // one-lane algebra (4 x 4 inverse before a warp, motion filter after the IRLS, 3 x 3 inverse at the
        SplatWin win;  // end of the solve) is used while neither is, and so are the fp64 sums of pass 1
        double dwork[36 * 3 + 32];
        double p1[27][P1_SETS];
#if SF_REFORDER
        RoChunk ro;    // reference-order build: a chunk of the ordered per-cluster sums
        RoChunk2 ro2;  // ... with the two residuals of every pixel (`ro2.c` IS `ro`)
        RoRows rows;   // ... a chunk of weighted rows for the row-by-row fp64 sums of pass 1
#endif
    };
    // reductions
    double red[SF_NW][28];
    float redf[SF_NW][2];
    int redi[SF_NW];
    long long lab_sum[SF_NC];
    long long prior_sum[SF_NC];
    int prior_size[SF_NC], prior_nonnull[SF_NC], valid_cnt[SF_NC];
    // stream state
    float T[16], Tinv[16];
    float twist[6], twist_level[6], twist_old[6];
    float est_cov[36];
    float b_segm[SF_NC], b_prior[SF_NC], lambda_t_w[SF_NC];
    unsigned conn[SF_NC];
    float kb;
    // IRLS
    float AtA[36], AtB[6], Var[6], prev_sol[6];
    float aver_res, aver_res_old, inv_max_c, inv_max_d, res_sqnorm;
    float last_delta;  // |Var - prev_sol|_inf of the last IRLS iteration (the trace reports it)
    double sq_total;  // ||res||^2 of the last pass 2, summed over the workgroups of the cluster
    int px_begin, px_end;  // pixel range of the level the streaming passes walk: this workgroup's share of the level
    int rec_slot;          // record slot the passes stream (the stream's, or this workgroup's private one)
    double init_abs_c, init_abs_d;  // sum of wc |dct| and wd |ddt| over validPixels (raw pre-weights), from the linearisation
    int n_valid, ctrl, status, n_irls, n_outer, first;
    long long pixel_iters;
    // small solves
    float M6[6 * 7], tmp6[6], y6[6];
    int tr6[6];
    union {
        float M24[SF_NC * (SF_NC + 1)];  // factored and used inside solve_irls
        SplatMarks marks;                // the warp's column watermarks (solve_warp, between two solve_irls)
    };
    float tmp24[SF_NC], y24[SF_NC], seg_diag[SF_NC], aver_res_label[SF_NC];
    int tr24[SF_NC];
    int seg_allzero;
    long long prof[SF_PROF_SLOTS], t_last;
};

#ifdef SF_NO_PROF_MARK
#define PROF_MARK(s, tid, slot) do {} while (0)
#else
#define PROF_MARK(s, tid, slot)                         \
    do {                                                \
        if ((tid) == 0) {                               \
            const long long now_ = wall_clock64();      \
            (s).prof[slot] += now_ - (s).t_last;        \
            (s).t_last = now_;                          \
        }                                               \
    } while (0)
#endif
