// sf_view_common.h — what the translation units that draw surfel maps from a free view share (sf_view.h: the kernels of
// include/sf_view.h; sf_score.h: the kernel of include/sf_score.h): the argument table of a view and whom a view culls. The
// camera transform, the sprite extent and the fragment test are those of the prediction: sf_surfel_geom.h, used on ViewArgs.
// No kernel is defined here.
#pragma once
#include "sf_surfel_geom.h"

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

// camera-frame position, normal and radius of surfel s; false if culled: depth range, confidence
// (!(s[3] < min_confidence) draws: a NaN confidence is drawn), age (test B of sfw_filter: a NaN s[7] is not drawn)
__device__ __forceinline__ bool sfv_to_camera(const ViewArgs &a, int s, PV3 &h, PV3 &n, float &rad) {
    float conf, tlast;
    const auto q = surfel_record(a, s);
    h = surfel_camera_position(a, q, conf, tlast);
    n = surfel_camera_normal(a, q, rad);  // every output is set, culled or not: the resolve and score kernels ignore the result
    if (h.z > a.max_depth || h.z < 0.4f || conf < a.min_confidence) return false;
    if (a.use_age && !(a.tick - tlast <= a.max_age)) return false;
    return true;
}

// what surfel s draws: camera-frame geometry and the clipped pixel rectangle [i0, i1] x [j0, j1] of its sprite; false: nothing
__device__ __forceinline__ bool sfv_sprite(const ViewArgs &a, int s, PV3 &h, PV3 &n, float &rad, int &i0, int &i1, int &j0, int &j1) {
    return sfv_to_camera(a, s, h, n, rad) && surfel_sprite(a, h, n, rad, i0, i1, j0, j1);
}
