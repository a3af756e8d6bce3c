// sf_closure_rules.h — the PER SAMPLE rule of include/sf_closure.h that the host and the device share: what one sample of a loop
// closure -- the winning surfel of the active part under the believed pose, the winning surfel of the old part under the refined
// pose, on one camera ray -- becomes: a LINK, a PIN, both or neither, with the predicates the counts are made of and the two
// quantised sums. Plain C++, fp32 in the written order, one operation per expression (no contraction: -ffp-contract=off), so the
// host (sfc_link_sample of sf_hip_closure.hip, and tests/cpp/closure_rules_host.cpp under the sanitizers) and the device
// (sf_closure.h) run the same text and give the same bits. It includes nothing of the library and defines no kernel.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SFC_HD __host__ __device__
#else
#define SFC_HD
#endif

// the bits of the mask (include/sf_closure.h: SFC_FOUND_*)
#define SFC_BIT_BOTH 1
#define SFC_BIT_NEAR 2
#define SFC_BIT_APART 4
#define SFC_BIT_LINK 8           // a LINK was written
#define SFC_BIT_PIN 16           // a PIN was written
#define SFC_BIT_LINK_DROPPED 32  // a LINK was made and held a value that is not finite
#define SFC_BIT_PIN_DROPPED 64   // likewise a PIN

struct SfcRecord {  // the constraint of include/sf_deform.h, field for field
    float src[3];
    float dst[3];
    float time;
    float weight;
};

struct SfcRule {  // what of the parameters a sample reads
    int pins;
    float gate_abs, gate_rel, min_time_gap, w_link, w_pin;
};

SFC_HD static inline bool sfc_finite(float v) { return fabsf(v) < INFINITY; }  // false for NaN
// src, dst and time; the weight is a checked parameter
SFC_HD static inline bool sfc_record_finite(const SfcRecord *c) {
    return sfc_finite(c->src[0]) && sfc_finite(c->src[1]) && sfc_finite(c->src[2]) && sfc_finite(c->dst[0]) && sfc_finite(c->dst[1]) && sfc_finite(c->dst[2]) &&
           sfc_finite(c->time);
}
// the quantisation of the two sums: 1/16384 m, clipped at 32 m
SFC_HD static inline long long sfc_quantise(float v) {
    const float clipped = fminf(v, 32.f);
    const float scaled = clipped * 16384.f;
    return (long long)rintf(scaled);
}

// One sample. sa / so: floats 0 .. 7 of the winning surfels (read only with has_a / has_o), zA / zO the depths of the two
// winning fragments, T = inverse(view_from.pose) as the drawing holds it and P = view_to.pose, both column-major. Returns the
// mask; *link and *pin are written only with their bits SFC_BIT_LINK and SFC_BIT_PIN; *q_dz and *q_shift are this sample's
// terms of sum_dz and sum_shift (0 when it has none).
SFC_HD static inline int sfc_link_core(bool has_a, const float *sa, bool has_o, const float *so, float zA, float zO, const float *T, const float *P,
                                       const SfcRule *r, SfcRecord *link, SfcRecord *pin, long long *q_dz, long long *q_shift) {
    int mask = 0;
    *q_dz = 0;
    *q_shift = 0;
    bool apart = false;
    if (has_a && has_o) {
        mask |= SFC_BIT_BOTH;
        const float diff = zA - zO;
        const float dz = fabsf(diff);
        const float rel = r->gate_rel * zO;
        const float gate = r->gate_abs + rel;
        if (dz <= gate) {
            mask |= SFC_BIT_NEAR;
            *q_dz = sfc_quantise(dz);
            const float gap = sa[6] - so[6];
            apart = gap > r->min_time_gap;
        }
    }
    if (apart) {
        mask |= SFC_BIT_APART;
        SfcRecord c;
        const float x = sa[0], y = sa[1], z = sa[2];
        c.src[0] = x;
        c.src[1] = y;
        c.src[2] = z;
        // h = T * src: the expression of surfel_camera_position (sf_surfel_geom.h)
        const float hx = T[0] * x + T[4] * y + T[8] * z + T[12];
        const float hy = T[1] * x + T[5] * y + T[9] * z + T[13];
        const float hz = T[2] * x + T[6] * y + T[10] * z + T[14];
        for (int k = 0; k < 3; k++) c.dst[k] = ((P[k] * hx + P[4 + k] * hy) + P[8 + k] * hz) + P[12 + k];
        c.time = sa[6];
        c.weight = r->w_link;
        if (sfc_record_finite(&c)) {
            mask |= SFC_BIT_LINK;
            *link = c;
            const float dx = c.dst[0] - c.src[0];
            const float dy = c.dst[1] - c.src[1];
            const float dzz = c.dst[2] - c.src[2];
            const float xx = dx * dx;
            const float yy = dy * dy;
            const float zz = dzz * dzz;
            const float xy = xx + yy;
            *q_shift = sfc_quantise(sqrtf(xy + zz));
        } else {
            mask |= SFC_BIT_LINK_DROPPED;
        }
    }
    const bool want_pin = r->pins == 1 ? apart : (r->pins == 2 ? has_o : false);
    if (want_pin) {
        SfcRecord c;
        for (int k = 0; k < 3; k++) {
            c.src[k] = so[k];
            c.dst[k] = so[k];
        }
        c.time = so[6];
        c.weight = r->w_pin;
        if (sfc_record_finite(&c)) {
            mask |= SFC_BIT_PIN;
            *pin = c;
        } else {
            mask |= SFC_BIT_PIN_DROPPED;
        }
    }
    return mask;
}

// SAMPLES: how many sample positions 0 <= s2 + i * s < extent there are, s2 = s / 2
SFC_HD static inline int sfc_samples_along(int extent, int stride) {
    const int s2 = stride / 2;
    return extent > s2 ? (extent - s2 + stride - 1) / stride : 0;
}
