// sf_splat.h — the forward splat of the warp and of the 5-frame residuals: fixed-point accumulator cells, the tiled
// splat through an LDS window (tiled_splat) and the normalisation of a cell when it is read. Only the stages that splat
// or read accumulator cells include this (sf_warp.h, sf_linearise.h, sf_residuals.h, sf_reforder.h).
#pragma once

#include "sf_device_common.h"

// ---------------------------------------------------------------------------------------------
//  forward splat of one source pixel (reference FrontEnd.cpp:808-868 / :960-1019): transform with T
//  (rows 0..2 of the inverse odometry, row-major 3x4), project to centi-pixels, distribute to the
//  1 or 4 neighbouring target pixels with integer weights.  Integer atomics: order independent.
// ---------------------------------------------------------------------------------------------
struct SplatGeom {
    float T[12];
    float f, disp_u_i, disp_v_i;
    int cols_lim, rows_lim, rows_i;
};

// a * w for a 64-bit fixed-point value |a| < 2^55 and a weight 0 <= w < 2^23: the low word times w as one 32 x 32 -> 64
// product, the (small, signed) high word through the 24-bit multiplier. Equal to the plain 64-bit product, in 3 instructions.
__device__ __forceinline__ long long mul_i64_w(long long a, int w) {
    const unsigned long long lo = (unsigned long long)(unsigned)a * (unsigned)w;
    const int hi = __mul24((int)(a >> 32), w) + (int)(lo >> 32);
    return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}
// the packed increment of an intensity cell, (w << ACC_W_SHIFT) + w * jf, for a 32-bit fixed-point intensity: one signed
// 32 x 32 -> 64 product, the weight added into the high word
__device__ __forceinline__ long long mul_packed_w(int jf, int w) {
    const long long p = (long long)jf * (long long)w;
    const int hi = (int)(p >> 32) + (w << (ACC_W_SHIFT - 32));
    return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)p);
}

// depth / intensity of a target pixel from its fixed-point accumulators: sum(w * value) / sum(w).
// The integer sums are exact; one int64 -> float conversion and one float division round twice
// (<= 1 ulp from the exact quotient, the same order as the reference's own float accumulation).
// The two quotients share the divisor (an integer in [1, 2^20], exact in float): one hardware reciprocal (1 ulp), refined
// by a Newton step, and a residual correction per quotient -- the correctly rounded quotient in all but a vanishing share
// of the cases, within 1 ulp always, at a third of the instructions of two IEEE division sequences.
__device__ __forceinline__ void normalise_acc(long long sd, long long packed, float &dw, float &iw) {
    const long long si = (long long)((unsigned long long)packed << (64 - ACC_W_SHIFT)) >> (64 - ACC_W_SHIFT);
    const float wf = (float)(unsigned)((packed - si) >> ACC_W_SHIFT);
    const float nd = (float)sd * (1.f / 67108864.f), ni = (float)si * (1.f / FIX_INTENS);
    float r = __builtin_amdgcn_rcpf(wf);
    r = fmaf(fmaf(-wf, r, 1.f), r, r);
    float q = nd * r;
    dw = fmaf(fmaf(-wf, q, nd), r, q);
    q = ni * r;
    iw = fmaf(fmaf(-wf, q, ni), r, q);
}

// ---------------------------------------------------------------------------------------------
//  Tiled splat: the level is walked in source tiles of SPLAT_TV x SPLAT_TU pixels.  The targets of
//  a tile fall into a small window of the warped image (a rigid warp is locally a shift), which is
//  accumulated in LDS with integer ds_add atomics and then added to the global accumulators once
//  per touched cell: ~3x fewer, fully coalesced global atomics than one global atomic triple per
//  bilinear tap.  Targets outside the window (strong local stretch) take the global path directly.
//  Integer sums => the result is independent of both orders.
// ---------------------------------------------------------------------------------------------
#define SPLAT_TV 64
#define SPLAT_TU ((SF_NT == 256 ? 4 : 2) * SF_NT / 64)
#define SPLAT_PX ((SPLAT_TV * SPLAT_TU) / SF_NT)  // source pixels per lane and tile
#define SPLAT_MARGIN 6  // window cells beyond the tile size in each direction (a rigid warp is locally a shift: rarely more)
#define WIN_V (SPLAT_TV + SPLAT_MARGIN)
#define WIN_U (SPLAT_TU + SPLAT_MARGIN)
#define WIN_CELLS (WIN_V * WIN_U)

#define SPLAT_MAX_LAZY_TILES 512
#define SPLAT_LAZY_COLS 640  // lazy mode keeps a row watermark per accumulator column (SplatMarks)
struct SplatWin {
    long long d[WIN_CELLS];
    long long i[WIN_CELLS];  // packed like the global cell
    int vmin, umin;
    int vmax, umax;  // lazy mode: the last row / column any tap of the tile can reach (the flush walks the touched box, not the window)
    unsigned ovf[SPLAT_MAX_LAZY_TILES / 32];  // lazy mode: tiles with targets outside their window (replayed at the end)
};
// Lazy initialisation (one workgroup per stream only): no pass zeroes the accumulator image before the splat. A watermark
// per accumulator COLUMN (SplatMarks: rows [0, zrow[c]) of column c hold zero or sums) tells the flush of a window which
// of its cells nobody has written yet: those are STORED -- the window's value, zero included -- and only cells below the
// watermark, which an earlier window reached, take atomics; rows between the watermark and the window's first row are
// stored as zero, and what no window reached is zeroed after the last tile. A cell then crosses the fabric once on its way
// out (the L2 writes stores through and gives a line up after an atomic: zero + atomic cost two write-backs and a fetch)
// instead of being zeroed first and added to afterwards. The tiles walk down a strip of SPLAT_TU columns and then move
// right, so the watermark of a column only grows. Targets outside a tile's window (rare: strong local stretch) cannot go
// straight to the global cells -- their cell may not be initialised yet -- so the tile is flagged and replayed after the
// last tile.
struct SplatMarks {
    unsigned short zrow[SPLAT_LAZY_COLS];
};
__device__ __forceinline__ bool splat_lazy_ok(int rows_i, int cols_i, int G) {
    const int tiles = ((rows_i + SPLAT_TV - 1) / SPLAT_TV) * ((cols_i + SPLAT_TU - 1) / SPLAT_TU);
    return G == 1 && tiles <= SPLAT_MAX_LAZY_TILES && cols_i <= SPLAT_LAZY_COLS && rows_i < 65536;
}

// Src::load(v, u, idx, z, xr, yr, iw) -> bool valid
template <class Src>
__device__ __forceinline__ void tiled_splat(const SplatGeom &g, int rows_i, int cols_i, const Src &src, gptr<long long> acc_d,
                                            gptr<long long> acc_i, LDS SplatWin &win, LDS SplatMarks &marks, int tid, int tile_first = 0,
                                            int tile_step = 1, bool lazy = false, long long *replayed = nullptr) {
    const int lane = tid & 63;
    const int tiles_v = (rows_i + SPLAT_TV - 1) / SPLAT_TV, tiles_u = (cols_i + SPLAT_TU - 1) / SPLAT_TU;
    const int n_tiles = tiles_v * tiles_u;
    if (lazy) {
        if (tid < SPLAT_MAX_LAZY_TILES / 32) win.ovf[tid] = 0;  // ordered before its first use by the tile loop's barriers
        for (int c = tid; c < cols_i; c += SF_NT) marks.zrow[c] = 0;
    }
    // the rows [from, to) of column c, for every lane that raises `flag`, zeroed by the whole wave (call it wave-uniformly)
    auto zero_flagged = [&](bool flag, int c, int from, int to) {
        for (unsigned long long m = __ballot(flag); m; m &= m - 1) {
            const int l = __builtin_ctzll(m);
            const int cc = __builtin_amdgcn_readlane(c, l), tt = __builtin_amdgcn_readlane(to, l);
            for (int v = __builtin_amdgcn_readlane(from, l) + lane; v < tt; v += 64) {
                gst(acc_d, v + cc * rows_i, 0ll);
                gst(acc_i, v + cc * rows_i, 0ll);
            }
        }
    };
    int pend_u0 = -1, pend_nu = 0, pend_z = 0;  // the columns the last flush reached and their new watermark (set one trip later: no barrier of its own)
    // lazy: a second walk over the tiles (it >= n_tiles) replays the flagged ones for their out-of-window targets
    for (int it = tile_first; it < (lazy ? 2 * n_tiles : n_tiles); it += tile_step) {  // a cluster's workgroups take every G-th tile
        const bool replay = it >= n_tiles;
        if (pend_u0 >= 0) {  // (the flush that read the watermarks ended with a barrier)
            if (tid < pend_nu && pend_u0 + tid < cols_i && pend_z > (int)marks.zrow[pend_u0 + tid]) marks.zrow[pend_u0 + tid] = (unsigned short)pend_z;
            pend_u0 = -1;
        }
        const int tile = replay ? it - n_tiles : it;
        if (replay) {
            if (it == n_tiles) {  // every tile flushed: zero what no window reached; the flags are complete
                __syncthreads();  // the last window's watermarks (set at the top of this trip) are visible
                for (int c0 = 0; c0 < cols_i; c0 += SF_NT) {  // a lane per column; a column short of the last row is rare
                    const int c = c0 + tid;
                    const int z = c < cols_i ? (int)marks.zrow[c] : rows_i;
                    zero_flagged(z < rows_i, c, z, rows_i);
                }
                __syncthreads();
            }
            if (!((uniform_i((int)win.ovf[tile >> 5]) >> (tile & 31)) & 1)) continue;
            if (tid == 0 && replayed) *replayed += 1;  // diagnostic counter (slot 24 of sf_get_stage_profile)
        }
        const int tv0 = (tile % tiles_v) * SPLAT_TV, tu0 = (tile / tiles_v) * SPLAT_TU;
        // ---- phase 1: clear the window, load + project this lane's source pixels, window origin
        for (int q = tid; q < WIN_CELLS; q += SF_NT) {
            win.d[q] = 0;
            win.i[q] = 0;
        }
        if (tid == 0) {
            win.vmin = 0x7fffffff;
            win.umin = 0x7fffffff;
            win.vmax = -1;
            win.umax = -1;
        }
        // target pixel (qu, qv) and the centi-pixel offsets (ru, rv) inside it: uwarp = 100 qu + ru (reference FrontEnd.cpp:819-853)
        int qu[SPLAT_PX], ru[SPLAT_PX], qv[SPLAT_PX], rv[SPLAT_PX];
        long long dfix[SPLAT_PX];
        int ifix[SPLAT_PX];
        bool ok[SPLAT_PX];
        float z[SPLAT_PX], xr[SPLAT_PX], yr[SPLAT_PX], iw[SPLAT_PX];
#pragma unroll
        for (int k = 0; k < SPLAT_PX; k++) {
            const int v = tv0 + lane, u = tu0 + (tid >> 6) + k * (SF_NT / 64);
            const bool inside = v < rows_i && u < cols_i;
            const int idx = inside ? v + u * rows_i : 0;
            ok[k] = src.load(v, u, idx, z[k], xr[k], yr[k], iw[k]) && inside;
        }
        int vtop = 0, utop = 0;  // max over the lane's valid pixels of INT_MAX - q (q >= 0): the wave maximum gives the minimum
        int vbot = 0, ubot = 0;  // ... and of q + 2 (0: no valid pixel): the last row / column a tap can reach, + 1
#pragma unroll
        for (int k = 0; k < SPLAT_PX; k++) {
            const float x_w = g.T[0] * xr[k] + g.T[1] * yr[k] + g.T[2] * z[k] + g.T[3];
            const float y_w = g.T[4] * xr[k] + g.T[5] * yr[k] + g.T[6] * z[k] + g.T[7];
            const float depth_w = g.T[8] * xr[k] + g.T[9] * yr[k] + g.T[10] * z[k] + g.T[11];
            const int uw = cvt_trunc_x86(100.f * (g.f * x_w / depth_w + g.disp_u_i));
            const int vw = cvt_trunc_x86(100.f * (g.f * y_w / depth_w + g.disp_v_i));
            ok[k] = ok[k] && (uw >= 0) && (uw < g.cols_lim) && (vw >= 0) && (vw < g.rows_lim);
            const unsigned uu = ok[k] ? (unsigned)uw : 0u, vv = ok[k] ? (unsigned)vw : 0u;  // non-negative: unsigned division
            qu[k] = (int)(uu / 100u);
            ru[k] = (int)(uu - 100u * (unsigned)qu[k]);
            qv[k] = (int)(vv / 100u);
            rv[k] = (int)(vv - 100u * (unsigned)qv[k]);
            dfix[k] = to_fix(depth_w, FIX_DEPTH, 1000.f);
            ifix[k] = to_fix_i32(iw[k], FIX_INTENS, 4.f);
            if (ok[k]) {
                vtop = max(vtop, 0x7fffffff - qv[k]);
                utop = max(utop, 0x7fffffff - qu[k]);
                vbot = max(vbot, qv[k] + 2);
                ubot = max(ubot, qu[k] + 2);
            }
        }
        SF_DPP_REDUCE(vtop, dpp_i32, sf_op_maxi)
        SF_DPP_REDUCE(utop, dpp_i32, sf_op_maxi)
        const int vmin = 0x7fffffff - __builtin_amdgcn_readlane(vtop, 63), umin = 0x7fffffff - __builtin_amdgcn_readlane(utop, 63);
        int vlast = 0, ulast = 0;
        if (lazy) {  // (uniform)
            SF_DPP_REDUCE(vbot, dpp_i32, sf_op_maxi)
            SF_DPP_REDUCE(ubot, dpp_i32, sf_op_maxi)
            vlast = __builtin_amdgcn_readlane(vbot, 63) - 1;
            ulast = __builtin_amdgcn_readlane(ubot, 63) - 1;
        }
        __syncthreads();  // window cleared, origin initialised
        if (lane == 0) {
            lds_min(&win.vmin, vmin);
            lds_min(&win.umin, umin);
            if (lazy) {
                __hip_atomic_fetch_max(&win.vmax, vlast, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_max(&win.umax, ulast, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        __syncthreads();
        const int wv0 = uniform_i(win.vmin), wu0 = uniform_i(win.umin);
        bool outside = false;  // lazy: this lane had a target outside the window
        // ---- phase 2: splat into the window (LDS atomics), or straight to global if outside
        auto add = [&](int v, int u, int w, long long df, int jf) {
            const int dv = v - wv0, du = u - wu0;
            if (dv >= 0 && dv < WIN_V && du >= 0 && du < WIN_U) {
                if (!replay) {
                    const int c = dv + du * WIN_V;
                    lds_add(&win.d[c], mul_i64_w(df, w));
                    lds_add(&win.i[c], mul_packed_w(jf, w));
                }
            } else if (lazy && !replay) {
                outside = true;
            } else {
                const int t = v + u * g.rows_i;
                gatomic_add_at(acc_d, t, mul_i64_w(df, w));
                gatomic_add_at(acc_i, t, mul_packed_w(jf, w));
            }
        };
#pragma unroll
        for (int k = 0; k < SPLAT_PX; k++) {
            if (!ok[k]) continue;
            const int delta_l = ru[k], delta_r = 100 - ru[k], delta_d = rv[k], delta_u = 100 - rv[k];
            const long long df = dfix[k];
            const int jf = ifix[k];
            if (min(delta_r, delta_l) + min(delta_u, delta_d) < 5) {  // within 5 centi-pixels of a pixel centre
                add(delta_u > delta_d ? qv[k] : qv[k] + 1, delta_r > delta_l ? qu[k] : qu[k] + 1, 200, df, jf);
            } else {
                const int dv0 = qv[k] - wv0, du0 = qu[k] - wu0;  // >= 0: the window origin is the tile's minimum
                if (dv0 < WIN_V - 1 && du0 < WIN_U - 1) {        // the 2 x 2 block lies in the window: one test, four fixed offsets
                    if (replay) continue;
                    const int c = dv0 + du0 * WIN_V;
                    const int w11 = delta_l + delta_d, w10 = delta_r + delta_d, w01 = delta_l + delta_u, w00 = delta_r + delta_u;
                    lds_add(&win.d[c + WIN_V + 1], mul_i64_w(df, w11));
                    lds_add(&win.i[c + WIN_V + 1], mul_packed_w(jf, w11));
                    lds_add(&win.d[c + 1], mul_i64_w(df, w10));
                    lds_add(&win.i[c + 1], mul_packed_w(jf, w10));
                    lds_add(&win.d[c + WIN_V], mul_i64_w(df, w01));
                    lds_add(&win.i[c + WIN_V], mul_packed_w(jf, w01));
                    lds_add(&win.d[c], mul_i64_w(df, w00));
                    lds_add(&win.i[c], mul_packed_w(jf, w00));
                } else {
                    add(qv[k] + 1, qu[k] + 1, delta_l + delta_d, df, jf);
                    add(qv[k] + 1, qu[k], delta_r + delta_d, df, jf);
                    add(qv[k], qu[k] + 1, delta_l + delta_u, df, jf);
                    add(qv[k], qu[k], delta_r + delta_u, df, jf);
                }
            }
        }
        if (lazy && !replay && __any(outside)) {
            if (lane == 0) lds_or(&win.ovf[tile >> 5], 1u << (tile & 31));
        }
        __syncthreads();
        // ---- phase 3: add the touched cells to the global accumulators (consecutive lanes -> consecutive v)
        if (lazy) {
            if (!replay && wu0 != 0x7fffffff) {  // (no valid source pixel in the tile: nothing to flush, no column reached)
                // Groups of 16 lanes take 16 rows that start on a multiple of 16 (a 128-byte line of cells where the level's
                // rows are a multiple of 16, as at QVGA's level 0): the stores are whole lines, written once. Rows [r0, znew)
                // of every window column: the window's cells and the padding up to the next multiple of 16 either side.
                // (round 5) only the box the tile's taps can have reached -- a rigid warp moves a 64 x 16 tile into about 66 x 18 cells of
                // its 70 x 22 window --: what lies beyond it in the window holds zeros that nobody needs to write now (the
                // watermarks say what is initialised; a later window, or the sweep after the last tile, takes care of the rest)
                const int vreach = min(wv0 + WIN_V, uniform_i(win.vmax) + 1);
                const int ureach = min(WIN_U, uniform_i(win.umax) + 1 - wu0);
                const int vend = min(vreach, rows_i);
                const int znew = min((vend + 15) & ~15, rows_i), r0 = wv0 & ~15;
                const int ng = (znew - r0 + 15) >> 4;  // groups per column
                // gi / ng == (gi * mdiv) >> 16 for gi * ng < 65536 (mdiv = floor(65536 / ng) + 1; the quotient is far from an
                // integer unless ng is a power of two, where the reciprocal is exact)
                const unsigned mdiv = (unsigned)(65536.f * __builtin_amdgcn_rcpf((float)ng)) + 1u;
                const int ncols = min(ureach, cols_i - wu0);
                const int total = ng * ncols;
                for (int g0 = 0; g0 < total; g0 += SF_NT / 16) {  // (wave-uniform trip count: zero_flagged wants the whole wave)
                    const int gi = g0 + (tid >> 4);
                    const int du = (int)(((unsigned)gi * mdiv) >> 16), gr = gi - du * ng;
                    const int c = wu0 + du, v = r0 + (gr << 4) + (tid & 15);
                    const bool live = gi < total && v < znew;
                    const int z = live ? (int)marks.zrow[c] : 0x7fff;
                    const int dv = v - wv0;
                    const bool in_win = live && dv >= 0 && v < vend;
                    const int q = in_win ? dv + du * WIN_V : 0;
                    const long long packed = in_win ? win.i[q] : 0ll, sd = in_win ? win.d[q] : 0ll;
                    const int t = v + c * g.rows_i;
                    if (live && v >= z) {  // nobody has written this cell: the window's value -- or zero -- is its value
                        gst(acc_d, t, sd);
                        gst(acc_i, t, packed);
                    } else if (packed != 0) {
                        gatomic_add_at(acc_d, t, sd);
                        gatomic_add_at(acc_i, t, packed);
                    }
                    // rows between the watermark and r0 (a column the window above did not reach): the first lane of the column's
                    // first group reports it
                    zero_flagged(live && gr == 0 && (tid & 15) == 0 && z < r0, c, z, r0);
                }
                pend_u0 = wu0;
                pend_nu = ncols;
                pend_z = znew;
            }
        } else if (!replay)
        for (int q = tid; q < WIN_CELLS; q += SF_NT) {
            const long long packed = win.i[q];
            if (packed == 0) continue;  // sum(w) >= 1 makes a touched cell non-zero
            const int du = q / WIN_V, dv = q - du * WIN_V;
            const int t = (wv0 + dv) + (wu0 + du) * g.rows_i;
            gatomic_add_at(acc_d, t, win.d[q]);
            gatomic_add_at(acc_i, t, packed);
        }
        __syncthreads();  // before the next tile clears the window
    }
}
