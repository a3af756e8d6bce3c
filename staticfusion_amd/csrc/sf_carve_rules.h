// sf_carve_rules.h — the rules OBSERVE and DECIDE of include/sf_carve.h that the host and the device share: what one surfel of a
// map is against one entry (a view with a depth frame) -- UNSEEN, THROUGH, SUPPORTED or OCCLUDED, with the three pixel counts of
// its window -- and whether the votes of all entries of its map carve it. Plain C++, fp32 in the written order, one operation per
// expression (no contraction: -ffp-contract=off), no square root, so the host (sfe_observe / sfe_decide of sf_hip_carve.hip, and
// tests/cpp/carve_rules_host.cpp under the sanitizers) and the device (sf_carve.h) run the same text and give the same bits. It
// includes nothing of the library and defines no kernel. The frame pointer is a template parameter only so that the device can
// hand in a pointer to global memory.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SFE_HD __host__ __device__
#else
#define SFE_HD
#endif

// the classes (include/sf_carve.h: SFE_CLASS_*)
#define SFE_UNSEEN 0
#define SFE_THROUGH 1
#define SFE_SUPPORTED 2
#define SFE_OCCLUDED 3

struct SfeRule {  // what of the parameters a surfel reads
    float tol_abs, tol_rel, z_max, min_cos;
    int window, min_pixels, min_votes, max_support;
};

struct SfeView {  // what of an entry's view a surfel reads, with the tick of the entry's map
    float t_inv[16];  // inverse(view.pose), column-major
    float cx, cy, fx, fy, max_depth, min_confidence;
    float tick, max_age;  // (float)tick of the map, (float)max_age
    int use_age;          // max_age >= 0
    int rows, cols;
};

// pdot of sf_surfel_geom.h
SFE_HD static inline float sfe_dot(float ax, float ay, float az, float bx, float by, float bz) { return ax * bx + ay * by + az * bz; }

// OBSERVE: surfel s (12 floats) against one entry; zf is the depth frame, rows x cols column-major. found[0..2] = through, near,
// front of the window (all 0 when the surfel never reaches the window). Returns the class.
template <class ZP>
SFE_HD static inline int sfe_observe_core(const float *s, const SfeView *v, ZP zf, const SfeRule *r, int *found) {
    found[0] = 0;
    found[1] = 0;
    found[2] = 0;
    const float *T = v->t_inv;
    const float hx = ((T[0] * s[0] + T[4] * s[1]) + T[8] * s[2]) + T[12];
    const float hy = ((T[1] * s[0] + T[5] * s[1]) + T[9] * s[2]) + T[13];
    const float hz = ((T[2] * s[0] + T[6] * s[1]) + T[10] * s[2]) + T[14];
    const float mx = (T[0] * s[8] + T[4] * s[9]) + T[8] * s[10];
    const float my = (T[1] * s[8] + T[5] * s[9]) + T[9] * s[10];
    const float mz = (T[2] * s[8] + T[6] * s[9]) + T[10] * s[10];
    // whom the view culls (sf_view_common.h: sfv_to_camera)
    if (hz > v->max_depth || hz < 0.4f || s[3] < v->min_confidence) return SFE_UNSEEN;
    if (v->use_age && !(v->tick - s[7] <= v->max_age)) return SFE_UNSEEN;
    const float d = sfe_dot(mx, my, mz, hx, hy, hz);
    const float mm = sfe_dot(mx, my, mz, mx, my, mz);
    const float hh = sfe_dot(hx, hy, hz, hx, hy, hz);
    const float c2 = r->min_cos * r->min_cos;
    const float mh = mm * hh;
    const float dd = d * d;
    const float bound = c2 * mh;
    if (!(d < 0.f && dd >= bound)) return SFE_UNSEEN;  // faces the camera, not grazing
    const float px = (v->fx * hx) / hz;
    const float py = (v->fy * hy) / hz;
    const float qx = (px + v->cx) + 0.5f;
    const float qy = (py + v->cy) + 0.5f;
    if (!(qx >= 0.f && qx < (float)v->cols && qy >= 0.f && qy < (float)v->rows)) return SFE_UNSEEN;
    const int i = (int)floorf(qx), j = (int)floorf(qy);
    const int w = r->window;
    const int i0 = i - w < 0 ? 0 : i - w, i1 = i + w > v->cols - 1 ? v->cols - 1 : i + w;
    const int j0 = j - w < 0 ? 0 : j - w, j1 = j + w > v->rows - 1 ? v->rows - 1 : j + w;
    int through = 0, near = 0, front = 0;
    for (int ii = i0; ii <= i1; ii++) {
        const float lx = ((float)ii - v->cx) / v->fx;
        const float lxm = lx * mx;
        for (int jj = j0; jj <= j1; jj++) {
            const float z = zf[jj + ii * v->rows];  // rows * cols <= 2^24
            const float ly = ((float)jj - v->cy) / v->fy;
            const float lym = ly * my;
            const float den = (lxm + lym) + mz;
            const float zp = d / den;
            const bool valid = z > 0.f && z <= r->z_max && zp >= 0.4f && zp <= v->max_depth;
            const float rel = r->tol_rel * zp;
            const float tol = r->tol_abs + rel;
            const float res = z - zp;
            through += (valid && res > tol) ? 1 : 0;
            near += (valid && fabsf(res) <= tol) ? 1 : 0;
            front += (valid && res < -tol) ? 1 : 0;
        }
    }
    found[0] = through;
    found[1] = near;
    found[2] = front;
    if (near > 0) return SFE_SUPPORTED;
    if (through >= r->min_pixels) return SFE_THROUGH;
    if (front > 0) return SFE_OCCLUDED;
    return SFE_UNSEEN;
}

// DECIDE: the votes of the entries of a surfel's map
SFE_HD static inline bool sfe_decide_core(int v_through, int v_support, const SfeRule *r) { return v_through >= r->min_votes && v_support <= r->max_support; }
