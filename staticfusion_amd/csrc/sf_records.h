// sf_records.h — reading the record planes the linearisation writes: vector loads of pixel pairs and the per-level
// constants from which a pixel's rows are rebuilt. Used by the segmentation prior (sf_linearise.h) and the passes (sf_irls.h).
#pragma once

#include "sf_device_common.h"

// Records are read through GLOBAL address-space pointers (global_load_*, not flat_load_*) and
// SF_VEC consecutive pixels per lane (8- or 16-byte loads: more bytes in flight per wave).
typedef __attribute__((address_space(1))) const float gcfloat;
typedef __attribute__((address_space(1))) const uint8_t gcu8;
typedef __attribute__((address_space(1))) const vfloat2 gcfloat2;
typedef __attribute__((address_space(1))) const vfloat4 gcfloat4;
typedef __attribute__((address_space(1))) const unsigned short gcu16;
typedef __attribute__((address_space(1))) const unsigned int gcu32;

struct RecPtrs {
    int with_labels;
    gcfloat *p[R_COUNT];
    gcfloat *dnew;  // NEW depth of the level (pyramid plane)
    gcu8 *lab;
};

// base (uniform, SGPR pair) + 32-bit unsigned byte offset (one VGPR shared by all planes): the
// saddr + voffset form of global_load, no 64-bit per-plane address arithmetic in the loop
typedef __attribute__((address_space(1))) const char gcchar;
// NT: the load policy, a compile-time property of the load. false: the default policy (the line is kept in L2 and in the
// memory-side cache); true: non-temporal (global_load ... nt, the same address form): for bytes nobody reads again before
// the caches have turned over, so that they do not displace the lines somebody will (the passes: sf_irls.h, pass_division)
template <bool NT, class V, class P>
__device__ __forceinline__ V load_policy(P *q) {
    if constexpr (NT)
        return __builtin_nontemporal_load(q);
    else
        return *q;
}
template <int VEC, bool NT = false>
__device__ __forceinline__ void load_plane(gcfloat *p, int idx0, float (&out)[VEC]) {
    const unsigned boff = (unsigned)idx0 * 4u;
    gcchar *q = (gcchar *)p + boff;
    if constexpr (VEC == 1) {
        out[0] = load_policy<NT, float>((gcfloat *)q);
    } else if constexpr (VEC == 2) {
        const vfloat2 v = load_policy<NT, vfloat2>((gcfloat2 *)q);
        out[0] = v.x;
        out[1] = v.y;
    } else {
        const vfloat4 v = load_policy<NT, vfloat4>((gcfloat4 *)q);
        out[0] = v.x;
        out[1] = v.y;
        out[2] = v.z;
        out[3] = v.w;
    }
}
template <int VEC, bool NT = false>
__device__ __forceinline__ void load_labels(gcu8 *p, int idx0, int (&out)[VEC]) {
    gcchar *q = (gcchar *)p + (unsigned)idx0;
    if constexpr (VEC == 1) {
        out[0] = load_policy<NT, uint8_t>((gcu8 *)q);
    } else if constexpr (VEC == 2) {
        const unsigned v = load_policy<NT, unsigned short>((gcu16 *)q);
        out[0] = v & 255u;
        out[1] = v >> 8;
    } else {
        const unsigned v = load_policy<NT, unsigned>((gcu32 *)q);
        out[0] = v & 255u;
        out[1] = (v >> 8) & 255u;
        out[2] = (v >> 16) & 255u;
        out[3] = v >> 24;
    }
}

template <int VEC>
struct RecVec {
    float v[R_COUNT][VEC];
    float dn[VEC];
    unsigned labraw;  // the VEC label bytes as loaded; unpacked at the point of use (rec_label)
    int lab[VEC];
};
// (the record planes, the new-depth plane and the label plane of a record share one policy)
template <int VEC, bool NT = false>
__device__ __forceinline__ void load_rec(const RecPtrs &rp, int idx0, RecVec<VEC> &r) {
    static_assert(VEC == 2, "the passes walk pixel pairs");
    // uniform: without segmentation every valid pixel belongs to cluster 0 and the plane is not read. The bytes are kept
    // as loaded: unpacking them here, inside the branch, made the compiler wait for the load (s_waitcnt vmcnt(0)) BEFORE
    // the other seven loads of the record were issued -- two memory round trips per trip of the loop
    unsigned raw = 0;
    if (rp.with_labels) raw = load_policy<NT, unsigned short>((gcu16 *)((gcchar *)rp.lab + (unsigned)idx0));
    r.labraw = raw;
    load_plane<VEC, NT>(rp.dnew, idx0, r.dn);
#pragma unroll
    for (int q = 0; q < R_COUNT; q++) load_plane<VEC, NT>(rp.p[q], idx0, r.v[q]);
}

// Per-level constants needed to rebuild a pixel's rows from its compact record.
struct LevelGeom {
    int rows_i;
    float inv_rows;   // 1/rows_i, to split a flat index into (v, u)
    float disp_u_i, disp_v_i;
    float inv_f_pyr;  // 2 tan(fovh/2) / cols_i        (pyramid xx/yy, reference FrontEnd.cpp:378)
    float inv_f_w;    // 1 / (cols_i / (2 tan(fovh/2)))  (warp xx/yy,    reference FrontEnd.cpp:874)
    float f_inv;      // cols_i / (2 tan(fovh/2))       (reference :537; it is f)
    float kph, inv_max_c, inv_max_d;
    int first;        // Warped := Pred iteration: xxWarped / yyWarped use the pyramid formula
};

// split a flat column-major index into (column u, row v)
__device__ __forceinline__ void split_index(const LevelGeom &g, int idx, float &fu, float &fv) {
    int u = (int)((float)idx * g.inv_rows);
    if (u * g.rows_i > idx) u--;
    if ((u + 1) * g.rows_i <= idx) u++;
    fu = float(u);
    fv = float(idx - u * g.rows_i);
}
