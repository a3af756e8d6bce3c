// sf_body_map_rules.h — the per-surfel rules of include/sf_body_maps.h that the host and the device share: the PIXEL SURFEL of
// a pixel and its four neighbours, the MOVE of a surfel by a world motion, and the MERGE of a pixel surfel into a map surfel.
// Plain C++, fp32 in the written order, one operation per expression (no contraction: -ffp-contract=off), so the host
// (sfp_pixel_surfel and sfp_merge_surfel of sf_hip_body_maps.hip, and tests/cpp/body_map_rules_host.cpp under the sanitizers)
// and the device (sf_body_maps.h) run the same text and give the same bits. It includes nothing of the library and defines no
// kernel.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SFP_HD __host__ __device__
#else
#define SFP_HD
#endif

// the minimum the fusion uses: y where y < x, else x (a NaN y gives x)
SFP_HD static inline float sfp_min(float x, float y) { return y < x ? y : x; }

SFP_HD static inline float sfp_dot(const float *a, const float *b) {
    const float xx = a[0] * b[0];
    const float yy = a[1] * b[1];
    const float zz = a[2] * b[2];
    const float xy = xx + yy;
    return xy + zz;
}

// Row r of a column-major 4 x 4: ((M[r] * x + M[4 + r] * y) + M[8 + r] * z), and + M[12 + r] for a position.
SFP_HD static inline float sfp_row(const float *M, int r, float x, float y, float z, bool translate) {
    const float a = M[r] * x;
    const float b = M[4 + r] * y;
    const float c = M[8 + r] * z;
    const float ab = a + b;
    const float abc = ab + c;
    return translate ? abc + M[12 + r] : abc;
}

// BACK-PROJECTION: ((((float)u - cx) * z) / fx, (((float)v - cy) * z) / fy, z)
SFP_HD static inline void sfp_back_project(float cx, float cy, float fx, float fy, int v, int u, float z, float *P) {
    const float du = (float)u - cx;
    const float dv = (float)v - cy;
    const float xu = du * z;
    const float yv = dv * z;
    P[0] = xu / fx;
    P[1] = yv / fy;
    P[2] = z;
}

// A colour channel as a byte: q = floorf(x * 255.0f + 0.5f), the byte is q when 0 <= q <= 255 holds and 0 otherwise (a NaN).
SFP_HD static inline int sfp_channel_byte(float x) {
    const float scaled = x * 255.0f;
    const float q = floorf(scaled + 0.5f);
    return (q >= 0.0f && q <= 255.0f) ? (int)q : 0;
}

SFP_HD static inline float sfp_encode_colour(float r, float g, float b) {
    const int rgb = (sfp_channel_byte(r) << 16) + (sfp_channel_byte(g) << 8) + sfp_channel_byte(b);
    return (float)rgb;  // < 2^24: exact
}

// The three channels of an encoded colour c: k = (int)c when 0 <= c < 2^24 holds and 0 otherwise; byte / 255.0f each.
SFP_HD static inline void sfp_decode_colour(float c, float *rgb) {
    const int k = (c >= 0.0f && c < 16777216.0f) ? (int)c : 0;
    rgb[0] = (float)((k >> 16) & 0xFF) / 255.0f;
    rgb[1] = (float)((k >> 8) & 0xFF) / 255.0f;
    rgb[2] = (float)(k & 0xFF) / 255.0f;
}

// The normal of pixel (v, u) from its depth and its four neighbours' (z5: centre, (v, u - 1), (v, u + 1), (v - 1, u),
// (v + 1, u)) under the TARGET MODEL rule: false when the pixel has none. The caller has made sure the pixel is interior.
SFP_HD static inline bool sfp_pixel_normal(const float *z5, int v, int u, float cx, float cy, float fx, float fy, float z_max, float normal_dz, float *n) {
    const float z = z5[0];
    for (int k = 0; k < 5; k++)
        if (!(z5[k] > 0.0f && z5[k] <= z_max)) return false;
    for (int k = 1; k < 5; k++) {
        const float d = z5[k] - z;
        if (!(fabsf(d) <= normal_dz)) return false;
    }
    float pl[3], pr[3], pu[3], pd[3];
    sfp_back_project(cx, cy, fx, fy, v, u - 1, z5[1], pl);
    sfp_back_project(cx, cy, fx, fy, v, u + 1, z5[2], pr);
    sfp_back_project(cx, cy, fx, fy, v - 1, u, z5[3], pu);
    sfp_back_project(cx, cy, fx, fy, v + 1, u, z5[4], pd);
    const float a[3] = {pr[0] - pl[0], pr[1] - pl[1], pr[2] - pl[2]};
    const float b[3] = {pd[0] - pu[0], pd[1] - pu[1], pd[2] - pu[2]};
    const float c0a = a[1] * b[2], c0b = b[1] * a[2];
    const float c1a = a[2] * b[0], c1b = b[2] * a[0];
    const float c2a = a[0] * b[1], c2b = b[0] * a[1];
    const float c[3] = {c0a - c0b, c1a - c1b, c2a - c2b};
    const float cc = sfp_dot(c, c);
    if (!(cc > 0.0f && cc < INFINITY)) return false;
    const float s = sqrtf(cc);
    n[0] = c[0] / s;
    n[1] = c[1] / s;
    n[2] = c[2] / s;
    return true;
}

// PIXEL SURFEL of the interior pixel (v, u): false when it has no normal (out untouched), else the 12 floats
// (X, conf_new | colour, 1, time, time | N, radius). pose: camera-to-world, column-major.
SFP_HD static inline bool sfp_pixel_surfel_core(const float *z5, int v, int u, const float *pose, float cx, float cy, float fx, float fy, int r, int g, int b,
                                                float z_max, float normal_dz, float conf_new, float time, float *out) {
    float n[3], P[3];
    if (!sfp_pixel_normal(z5, v, u, cx, cy, fx, fy, z_max, normal_dz, n)) return false;
    sfp_back_project(cx, cy, fx, fy, v, u, z5[0], P);
    const float fsum = fx + fy;
    const float focal = fsum / 2.0f;
    const float zf = P[2] / focal;
    const float r0 = zf * 1.41421356237f;
    const float wide = 2.0f * r0;
    const float tilted = r0 / fabsf(n[2]);
    out[0] = sfp_row(pose, 0, P[0], P[1], P[2], true);
    out[1] = sfp_row(pose, 1, P[0], P[1], P[2], true);
    out[2] = sfp_row(pose, 2, P[0], P[1], P[2], true);
    out[3] = conf_new;
    out[4] = sfp_encode_colour((float)r / 255.0f, (float)g / 255.0f, (float)b / 255.0f);
    out[5] = 1.0f;
    out[6] = time;
    out[7] = time;
    out[8] = sfp_row(pose, 0, n[0], n[1], n[2], false);
    out[9] = sfp_row(pose, 1, n[0], n[1], n[2], false);
    out[10] = sfp_row(pose, 2, n[0], n[1], n[2], false);
    out[11] = sfp_min(wide, tilted);
    return true;
}

// MOVE: position (with the translation) and normal (without) of s through W, column-major 4 x 4; everything else as it is.
// out may be s.
SFP_HD static inline void sfp_move_core(const float *W, const float *s, float *out) {
    const float x = s[0], y = s[1], z = s[2], nx = s[8], ny = s[9], nz = s[10];
    for (int k = 3; k < 8; k++) out[k] = s[k];
    out[11] = s[11];
    out[0] = sfp_row(W, 0, x, y, z, true);
    out[1] = sfp_row(W, 1, x, y, z, true);
    out[2] = sfp_row(W, 2, x, y, z, true);
    out[8] = sfp_row(W, 0, nx, ny, nz, false);
    out[9] = sfp_row(W, 1, nx, ny, nz, false);
    out[10] = sfp_row(W, 2, nx, ny, nz, false);
}

SFP_HD static inline float sfp_blend(float w, float old_value, float new_value, float den) {
    const float scaled = w * old_value;
    const float sum = scaled + new_value;
    return sum / den;
}

// MERGE of the pixel surfel p into the (moved) map surfel s. out may be s.
SFP_HD static inline void sfp_merge_core(const float *s, const float *p, float gain, float max_weight, float time, float *out) {
    const float w = fminf(s[5], max_weight);
    const float den = w + 1.0f;
    float o[12];
    for (int k = 0; k < 3; k++) o[k] = sfp_blend(w, s[k], p[k], den);
    float n[3];
    for (int k = 0; k < 3; k++) n[k] = sfp_blend(w, s[8 + k], p[8 + k], den);
    const float nn = sfp_dot(n, n);
    if (nn > 0.0f && nn < INFINITY) {
        const float len = sqrtf(nn);
        for (int k = 0; k < 3; k++) o[8 + k] = n[k] / len;
    } else {
        for (int k = 0; k < 3; k++) o[8 + k] = s[8 + k];
    }
    o[11] = sfp_blend(w, s[11], p[11], den);
    float cs[3], cp[3];
    sfp_decode_colour(s[4], cs);
    sfp_decode_colour(p[4], cp);
    o[4] = sfp_encode_colour(sfp_blend(w, cs[0], cp[0], den), sfp_blend(w, cs[1], cp[1], den), sfp_blend(w, cs[2], cp[2], den));
    const float c = s[3];
    const float room = 1.0f - c;
    const float step = gain * room;
    o[3] = c + step;
    o[5] = s[5] + 1.0f;
    o[6] = s[6];
    o[7] = time;
    for (int k = 0; k < 12; k++) out[k] = o[k];
}
