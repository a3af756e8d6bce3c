// sf_surfel_geom.h — which pixels a surfel covers and which fragment wins: the geometry of IndexMap::combinedPredict
// (reference IndexMap.cpp:221-300; Shaders/splat.vert, combo_splat.frag), stated once for everything that draws surfels: the
// prediction (sf_predict.h), the views (sf_view.h) and the scores (sf_score.h); the fusion (sf_fusion.h) takes the 3-vector
// helpers. The functions are templates over the argument struct A of their caller (PredictArgs, ViewArgs), which has
//     surfels, t_inv[16], cx, cy, fx, fy, max_depth, rows, cols, rays.
// Whom a caller culls (confidence, age) is the caller's business: surfel_camera_position hands out what the predicates need.
// Every float expression repeats the shader's association; no contraction (-ffp-contract=off): bit-identical to the CPU
// oracle. No kernel is defined here, so any number of translation units may include it.
#pragma once
#include "sf_device_common.h"

struct PV3 { float x, y, z; };
__device__ __forceinline__ float pdot(PV3 a, PV3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ PV3 padd(PV3 a, PV3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ PV3 psub(PV3 a, PV3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ PV3 pmul(PV3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ PV3 pnormalize(PV3 a) {
    const float n = sqrtf(pdot(a, a));
    return {a.x / n, a.y / n, a.z / n};
}
__device__ __forceinline__ PV3 pcross(PV3 a, PV3 b) { return {a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y}; }

// gl_FragDepth is a positive float, its bit pattern monotonic: atomicMin on the key is GL_LESS, and the earlier surfel wins a tie
__device__ __forceinline__ unsigned long long surfel_key(float depth, int s) { return ((unsigned long long)__float_as_uint(depth) << 32) | (unsigned)s; }

// the view ray of pixel (i, j) (combo_splat.frag:37-39): what the ray tables hold
__device__ __forceinline__ PV3 surfel_view_ray(int i, int j, float cx, float cy, float fx, float fy) {
    const float fx_ = float(i) + 0.5f, fy_ = float(j) + 0.5f;  // gl_FragCoord
    return pnormalize(PV3{(fx_ - cx) / fx, (fy_ - cy) / fy, 1.0f});
}

// Surfel s in the camera frame (splat.vert:55,68), from its record q, in two halves: the prediction culls between them (a
// culled surfel costs no normal), a view behind them. A caller that uses h, n and rad of a surfel whatever its cull says
// (the winner of a pixel, evaluated again) must have set all three whenever the surfel passes.
template <class A>
__device__ __forceinline__ gptr<const float> surfel_record(const A &a, int s) {
    return as_global(a.surfels) + (size_t)s * 12;  // typed global pointer: global_load, not flat_load
}
// the position, and the confidence and last-seen tick the culls look at ...
template <class A>
__device__ __forceinline__ PV3 surfel_camera_position(const A &a, gptr<const float> q, float &conf, float &tlast) {
    const float *T = a.t_inv;
    const PV3 vp{q[0], q[1], q[2]};
    conf = q[3];
    tlast = q[7];
    return PV3{T[0] * vp.x + T[4] * vp.y + T[8] * vp.z + T[12], T[1] * vp.x + T[5] * vp.y + T[9] * vp.z + T[13],
               T[2] * vp.x + T[6] * vp.y + T[10] * vp.z + T[14]};
}
// ... and the normalised normal with the radius
template <class A>
__device__ __forceinline__ PV3 surfel_camera_normal(const A &a, gptr<const float> q, float &rad) {
    const float *T = a.t_inv;
    const PV3 nin{q[8], q[9], q[10]};
    const PV3 n = pnormalize(PV3{T[0] * nin.x + T[4] * nin.y + T[8] * nin.z, T[1] * nin.x + T[5] * nin.y + T[9] * nin.z,
                                 T[2] * nin.x + T[6] * nin.y + T[10] * nin.z});
    rad = q[11];
    return n;
}

// the clipped pixel rectangle [i0, i1] x [j0, j1] of the sprite of a surfel at h, n, rad (splat.vert:64-85); false: nothing
template <class A>
__device__ __forceinline__ bool surfel_sprite(const A &a, PV3 h, PV3 n, float rad, int &i0, int &i1, int &j0, int &j1) {
    const float fcols = float(a.cols), frows = float(a.rows);
    const float ndc_x = ((((a.fx * h.x) / h.z) + a.cx) - (fcols * 0.5f)) / (fcols * 0.5f);
    const float ndc_y = ((((a.fy * h.y) / h.z) + a.cy) - (frows * 0.5f)) / (frows * 0.5f);
    if (!(ndc_x >= -1.f && ndc_x <= 1.f && ndc_y >= -1.f && ndc_y <= 1.f)) return false;  // centre outside the image: not drawn
    const float xw = (ndc_x + 1.f) * (fcols * 0.5f), yw = (ndc_y + 1.f) * (frows * 0.5f);
    const PV3 x1 = pmul(pmul(pnormalize(PV3{n.y - n.z, -n.x, n.x}), rad), 1.41421356f);
    const PV3 y1 = pcross(n, x1);
    const PV3 c1 = padd(h, x1), c2 = padd(h, y1), c3 = psub(h, y1), c4 = psub(h, x1);
    const float p1x = ((a.fx * c1.x) / c1.z) + a.cx, p1y = ((a.fy * c1.y) / c1.z) + a.cy;
    const float p2x = ((a.fx * c2.x) / c2.z) + a.cx, p2y = ((a.fy * c2.y) / c2.z) + a.cy;
    const float p3x = ((a.fx * c3.x) / c3.z) + a.cx, p3y = ((a.fy * c3.y) / c3.z) + a.cy;
    const float p4x = ((a.fx * c4.x) / c4.z) + a.cx, p4y = ((a.fy * c4.y) / c4.z) + a.cy;
    const float xlo = fminf(p1x, fminf(p2x, fminf(p3x, p4x))), xhi = fmaxf(p1x, fmaxf(p2x, fmaxf(p3x, p4x)));
    const float ylo = fminf(p1y, fminf(p2y, fminf(p3y, p4y))), yhi = fmaxf(p1y, fmaxf(p2y, fmaxf(p3y, p4y)));
    const float xDiff = fabsf(xhi - xlo), yDiff = fabsf(yhi - ylo);
    const float size = fmaxf(0.f, fmaxf(xDiff, yDiff));
    if (!(size > 0.f)) return false;
    const float half = size * 0.5f;
    i0 = max(0, (int)ceilf(xw - half - 0.5f)); i1 = min(a.cols - 1, (int)floorf(xw + half - 0.5f));
    j0 = max(0, (int)ceilf(yw - half - 0.5f)); j1 = min(a.rows - 1, (int)floorf(yw + half - 0.5f));
    // The sprite is a SQUARE of the longer extent (splat.vert:85), but a fragment survives only inside the disc
    // (combo_splat.frag:47), and the disc lies inside the diamond whose corners were just projected: pixels outside
    // their bounding rectangle (+ 1 pixel against rounding at the rim) would be discarded anyway -- skip them. That
    // holds only while all four corners lie in front of the camera: the projection of a corner with z <= 0 is mirrored
    // and the rectangle no longer contains the disc's image (a tilted disc with rad sqrt(2) above the depth of its
    // centre). Such a surfel keeps the whole square, as the shaders draw it.
    if (c1.z > 0.f && c2.z > 0.f && c3.z > 0.f && c4.z > 0.f) {
        i0 = max(i0, (int)floorf(xlo - 1.5f)); i1 = min(i1, (int)ceilf(xhi + 0.5f));
        j0 = max(j0, (int)floorf(ylo - 1.5f)); j1 = min(j1, (int)ceilf(yhi + 0.5f));
    }
    return i0 <= i1 && j0 <= j1;
}

// combo_splat.frag:37-49,63 for the fragment at pixel (i, j); false = discard
template <class A>
__device__ __forceinline__ bool surfel_fragment(const A &a, PV3 h, PV3 n, float rad, int i, int j, float &z, float &depth) {
    // the view ray of the pixel (combo_splat.frag:37-39) does not depend on the surfel: five divisions and a square root per
    // fragment become one 16-byte load from a table built with the same expression (surfel_view_ray)
    const vfloat4 lr = as_global(a.rays)[j + (size_t)i * a.rows];
    const PV3 l{lr.x, lr.y, lr.z};
    const PV3 corrected = pmul(l, pdot(h, n) / pdot(l, n));
    const PV3 diff = psub(corrected, h);
    if (pdot(diff, diff) > rad * rad) return false;
    z = corrected.z;
    depth = (corrected.z / (2.f * a.max_depth)) + 0.5f;
    return depth >= 0.f && depth < 1.f;  // depth range clip, and GL_LESS against the cleared depth 1.0: a fragment AT 1.0 fails
}

// bounding box of the sprites a workgroup draws, in bb (LDS): i0, j0, i1, j1 -- complete for every lane on return, and
// bb[2] < bb[0] when no lane is valid
__device__ __forceinline__ void workgroup_sprite_box(int *bb, bool valid, int i0, int i1, int j0, int j1) {
    if (threadIdx.x == 0) {
        bb[0] = bb[1] = 0x7fffffff;
        bb[2] = bb[3] = -1;
    }
    __syncthreads();
    if (valid) {
        atomicMin(&bb[0], i0);
        atomicMin(&bb[1], j0);
        atomicMax(&bb[2], i1);
        atomicMax(&bb[3], j1);
    }
    __syncthreads();
}
