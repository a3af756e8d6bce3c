// sf_view_common.h — what the translation units that draw surfel maps share (sf_view.h: the kernels of include/sf_view.h;
// sf_score.h: the kernel of include/sf_score.h): the argument table of a view, and the camera transform, sprite extent and
// fragment test of IndexMap::combinedPredict exactly as sf_predict.h states them (splat.vert, combo_splat.frag), restated on
// ViewArgs because that header defines kernels and cannot be included twice. Every float expression repeats the association
// of sf_predict.h (no contraction). No kernel is defined here.
#pragma once
#include "sf_device_common.h"

struct ViewArgs {
    const float *surfels;  // count x 12
    int count;
    float t_inv[16];       // column-major
    float cx, cy, fx, fy, max_depth, min_confidence;
    float tick, max_age;   // (float)tick of the map, (float)max_age
    int use_age;           // max_age >= 0
    int shade;             // SFV_SHADE_*
    int rows, cols;
    unsigned long long *keys;  // rows x cols, column-major
    const vfloat4 *rays;       // per pixel, column-major: normalize((x + 0.5 - cx) / fx, (y + 0.5 - cy) / fy, 1)
    int *large_count;          // [1]: length of large_list
    int *large_list;           // [count]: surfels whose clipped sprite has more than SFV_LARGE_PIXELS pixels
    float *depth;              // rows x cols row-major, or null
    uint8_t *rgb;              // rows x cols x 3 row-major, or null
    int *index;                // rows x cols row-major, or null
};
struct ViewRayArgs {
    vfloat4 *rays;
    int rows, cols;
    float cx, cy, fx, fy;
};

#define SFV_EMPTY 0xffffffffffffffffull

struct VV3 { float x, y, z; };
__device__ __forceinline__ float vdot(VV3 a, VV3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ VV3 vadd(VV3 a, VV3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ VV3 vsub(VV3 a, VV3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ VV3 vmul(VV3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ VV3 vnormalize(VV3 a) {
    const float n = sqrtf(vdot(a, a));
    return {a.x / n, a.y / n, a.z / n};
}
__device__ __forceinline__ VV3 vcross(VV3 a, VV3 b) { return {a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y}; }

// camera-frame position, normal and radius of surfel s (splat.vert:55,68); false if culled: depth range, confidence
// (!(s[3] < min_confidence) draws: a NaN confidence is drawn), age (test B of sfw_filter: a NaN s[7] is not drawn)
__device__ __forceinline__ bool sfv_to_camera(const ViewArgs &a, int s, VV3 &h, VV3 &n, float &rad) {
    const auto q = as_global(a.surfels) + (size_t)s * 12;
    const float *T = a.t_inv;
    const VV3 vp{q[0], q[1], q[2]};
    const float conf = q[3], tlast = q[7];
    h = VV3{T[0] * vp.x + T[4] * vp.y + T[8] * vp.z + T[12], T[1] * vp.x + T[5] * vp.y + T[9] * vp.z + T[13],
            T[2] * vp.x + T[6] * vp.y + T[10] * vp.z + T[14]};
    const VV3 nin{q[8], q[9], q[10]};
    n = vnormalize(VV3{T[0] * nin.x + T[4] * nin.y + T[8] * nin.z, T[1] * nin.x + T[5] * nin.y + T[9] * nin.z,
                       T[2] * nin.x + T[6] * nin.y + T[10] * nin.z});
    rad = q[11];
    if (h.z > a.max_depth || h.z < 0.4f || conf < a.min_confidence) return false;
    if (a.use_age && !(a.tick - tlast <= a.max_age)) return false;
    return true;
}

// combo_splat.frag:37-49,63 for the fragment at pixel (i, j); false = discard
__device__ __forceinline__ bool sfv_fragment(const ViewArgs &a, VV3 h, VV3 n, float rad, int i, int j, float &z, float &depth) {
    const vfloat4 lr = as_global(a.rays)[j + (size_t)i * a.rows];
    const VV3 l{lr.x, lr.y, lr.z};
    const VV3 corrected = vmul(l, vdot(h, n) / vdot(l, n));
    const VV3 diff = vsub(corrected, h);
    if (vdot(diff, diff) > rad * rad) return false;
    z = corrected.z;
    depth = (corrected.z / (2.f * a.max_depth)) + 0.5f;
    return depth >= 0.f && depth < 1.f;
}

// what surfel s draws: camera-frame geometry and the clipped pixel rectangle [i0, i1] x [j0, j1] of its sprite
// (splat.vert:57-85 as sf_predict_splat_kernel states it); false: nothing
__device__ __forceinline__ bool sfv_sprite(const ViewArgs &a, int s, VV3 &h, VV3 &n, float &rad, int &i0, int &i1, int &j0, int &j1) {
    if (!sfv_to_camera(a, s, h, n, rad)) return false;
    const float fcols = float(a.cols), frows = float(a.rows);
    const float ndc_x = ((((a.fx * h.x) / h.z) + a.cx) - (fcols * 0.5f)) / (fcols * 0.5f);
    const float ndc_y = ((((a.fy * h.y) / h.z) + a.cy) - (frows * 0.5f)) / (frows * 0.5f);
    if (!(ndc_x >= -1.f && ndc_x <= 1.f && ndc_y >= -1.f && ndc_y <= 1.f)) return false;  // centre outside the image: not drawn
    const float xw = (ndc_x + 1.f) * (fcols * 0.5f), yw = (ndc_y + 1.f) * (frows * 0.5f);
    const VV3 x1 = vmul(vmul(vnormalize(VV3{n.y - n.z, -n.x, n.x}), rad), 1.41421356f);
    const VV3 y1 = vcross(n, x1);
    const VV3 c1 = vadd(h, x1), c2 = vadd(h, y1), c3 = vsub(h, y1), c4 = vsub(h, x1);
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
    // a fragment survives only inside the disc, which lies inside the diamond of the four projected corners: pixels outside
    // their bounding rectangle (+ 1 pixel against rounding at the rim) would be discarded anyway (sf_predict.h)
    i0 = max(i0, (int)floorf(xlo - 1.5f)); i1 = min(i1, (int)ceilf(xhi + 0.5f));
    j0 = max(j0, (int)floorf(ylo - 1.5f)); j1 = min(j1, (int)ceilf(yhi + 0.5f));
    return i0 <= i1 && j0 <= j1;
}
