// sf_register_rules.h — the rules SAMPLE, PAIR and the row of include/sf_register.h that the host and the device share: whether a
// source surfel is sampled, where the estimate puts it, which representative of the destination's voxel table is its partner, the
// gates, and the point-to-plane row, quantised and summed by sf_p2p_system.h. Plain C++, fp32 in the written order, one operation
// per expression (no contraction: -ffp-contract=off), so the host (sfg_linearise of sf_hip_register.hip, and
// tests/cpp/register_rules_host.cpp under the sanitizers) and the device (sf_register.h) run the same text and give the same bits.
// It includes nothing of the library beyond sf_join_key.h (the key, the rank, the hash) and sf_p2p_system.h, and defines no
// kernel. The table is a template parameter only so that the device can hand in pointers to global memory and load 16 bytes at a
// time; a table offers
//   slots, log2_slots, count      the size of the table and the number of surfels that filled it
//   key(slot), best(slot)         the two words of a slot (sf_voxel_table.h: the key or SFJ_EMPTY; the highest bid of the voxel)
//   quad(r, which)                floats 4 * which .. 4 * which + 3 of destination surfel r
#pragma once
#include <math.h>
#include <stdint.h>

#include "sf_join_key.h"
#include "sf_p2p_system.h"

#define SFG_HD SFJ_HD
#define SFG_SYSTEM_WORDS p2p::WORDS
#define SFG_NOT_PAIRED (-1)
#define SFG_NOT_SAMPLED (-2)
#define SFG_MAX_SAMPLED (1 << 24)

struct SfgF4 {
    float x, y, z, w;
};

struct SfgRule {  // what of the parameters a surfel reads
    float inv;    // 1.0f / cell
    float dist_max, min_cos, min_confidence;
    int use_conf;  // min_confidence > 0
    int stride;
};

// what a linearisation finds for one sampled surfel
struct SfgPair {
    int partner;   // the representative's index in the destination, or SFG_NOT_PAIRED
    bool outside;  // Q is outside the grid
    bool lost;     // a probe walk visited every slot, or a slot named a surfel the table was not filled from
    int a[6];      // the quantised row, |.| <= 2^18
    int rho;       // the quantised residual, |.| <= 2^16
};

SFG_HD static inline float sfg_pdot(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

// SAMPLE: the surfels e with e % stride == 0 reach this test with their confidence
SFG_HD static inline bool sfg_confident(const SfgRule &r, float confidence) { return !r.use_conf || confidence >= r.min_confidence; }

// row k of the estimate E (3 x 4 row-major, floats) applied to v; the last term for a position only
SFG_HD static inline float sfg_row(const float *E, int k, float x, float y, float z, bool translate) {
    const float a = E[4 * k] * x;
    const float b = E[4 * k + 1] * y;
    const float c = E[4 * k + 2] * z;
    const float ab = a + b;
    const float abc = ab + c;
    return translate ? abc + E[4 * k + 3] : abc;
}

// v / sqrtf(v . v): false unless 0 < v . v < INFINITY (the rule of sf_deform_rules.h)
SFG_HD static inline bool sfg_unit(float x, float y, float z, float *ox, float *oy, float *oz) {
    const float vv = sfg_pdot(x, y, z, x, y, z);
    if (!(vv > 0.0f && vv < INFINITY)) return false;
    const float len = sqrtf(vv);
    *ox = x / len;
    *oy = y / len;
    *oz = z / len;
    return true;
}

// -1 or +1: the side of its cell a scaled coordinate lies on
SFG_HD static inline int sfg_side(float p, float inv) {
    const float sc = p * inv;
    const float f = floorf(sc);
    const float frac = sc - f;
    return frac < 0.5f ? -1 : 1;
}

// The representative of the voxel with the biased cell indices (cx, cy, cz), each in 1 .. 2^21 - 1: its index, -1 for a voxel
// that is not occupied. The walk is bounded by the number of slots.
template <class Table>
SFG_HD static inline int sfg_representative(const Table &t, uint32_t cx, uint32_t cy, uint32_t cz, bool *lost) {
    const uint64_t key = ((uint64_t)cx << 42) | ((uint64_t)cy << 21) | (uint64_t)cz;
    const uint32_t mask = (uint32_t)t.slots - 1u;
    uint32_t slot = sfj_first_slot(key, t.log2_slots);
    for (int step = 0; step < t.slots; step++) {
        const uint64_t seen = t.key(slot);
        if (seen == SFJ_EMPTY) return -1;
        if (seen == key) {
            const uint32_t r = 0xFFFFFFFFu - (uint32_t)t.best(slot);  // (sfj_candidate: the lower word is ~index)
            if (r >= (uint32_t)t.count) {
                *lost = true;
                return -1;
            }
            return (int)r;
        }
        slot = (slot + 1u) & mask;
    }
    *lost = true;
    return -1;
}

// PAIR and the row of one sampled surfel with position p and normal m (the first three members of each) at the estimate E.
template <class Table>
SFG_HD static inline SfgPair sfg_pair_core(const Table &t, const SfgRule &r, const float *E, const SfgF4 &p, const SfgF4 &m) {
    SfgPair o;
    o.partner = SFG_NOT_PAIRED;
    o.outside = false;
    o.lost = false;
    o.rho = 0;
    for (int k = 0; k < 6; k++) o.a[k] = 0;
    const float Qx = sfg_row(E, 0, p.x, p.y, p.z, true);
    const float Qy = sfg_row(E, 1, p.x, p.y, p.z, true);
    const float Qz = sfg_row(E, 2, p.x, p.y, p.z, true);
    uint32_t cx = 0, cy = 0, cz = 0;
    if (!(sfj_cell_index(Qx, r.inv, &cx) && sfj_cell_index(Qy, r.inv, &cy) && sfj_cell_index(Qz, r.inv, &cz))) {
        o.outside = true;
        return o;
    }
    const int sx = sfg_side(Qx, r.inv), sy = sfg_side(Qy, r.inv), sz = sfg_side(Qz, r.inv);
    const uint32_t limit = 2u * (uint32_t)SFJ_Q_BIAS;  // a biased index in the grid lies in 1 .. 2^21 - 1
    int partner = -1;
    float dd = 0.0f, dx = 0.0f, dy = 0.0f, dz = 0.0f, conf = 0.0f;
    for (int a = 0; a < 2; a++) {
        const uint32_t nx = cx + (uint32_t)(a * sx);
        if (nx < 1u || nx >= limit) continue;
        for (int b = 0; b < 2; b++) {
            const uint32_t ny = cy + (uint32_t)(b * sy);
            if (ny < 1u || ny >= limit) continue;
            for (int c = 0; c < 2; c++) {
                const uint32_t nz = cz + (uint32_t)(c * sz);
                if (nz < 1u || nz >= limit) continue;
                const int rep = sfg_representative(t, nx, ny, nz, &o.lost);
                if (rep < 0) continue;
                const SfgF4 M = t.quad(rep, 0);
                const float ex = Qx - M.x;
                const float ey = Qy - M.y;
                const float ez = Qz - M.z;
                const float ee = sfg_pdot(ex, ey, ez, ex, ey, ez);
                if (partner < 0 || ee < dd) {
                    partner = rep;
                    dd = ee;
                    dx = ex;
                    dy = ey;
                    dz = ez;
                    conf = M.w;
                }
            }
        }
    }
    if (partner < 0) return o;                                  // 1
    if (r.use_conf && !(conf >= r.min_confidence)) return o;    // 2
    const float gate = r.dist_max * r.dist_max;
    if (!(dd <= gate)) return o;                                // 3
    const SfgF4 v = t.quad(partner, 2);
    float nx = 0.0f, ny = 0.0f, nz = 0.0f, ux = 0.0f, uy = 0.0f, uz = 0.0f;
    if (!sfg_unit(v.x, v.y, v.z, &nx, &ny, &nz)) return o;      // 4
    const float mx = sfg_row(E, 0, m.x, m.y, m.z, false);
    const float my = sfg_row(E, 1, m.x, m.y, m.z, false);
    const float mz = sfg_row(E, 2, m.x, m.y, m.z, false);
    if (!sfg_unit(mx, my, mz, &ux, &uy, &uz)) return o;         // 5
    if (!(sfg_pdot(ux, uy, uz, nx, ny, nz) >= r.min_cos)) return o;  // 6
    const float res = sfg_pdot(nx, ny, nz, dx, dy, dz);
    if (!(fabsf(res) <= r.dist_max)) return o;                  // 7
    const float yz = Qy * nz, zy = ny * Qz;
    const float zx = Qz * nx, xz = nz * Qx;
    const float xy = Qx * ny, yx = nx * Qy;
    const float J[6] = {yz - zy, zx - xz, xy - yx, nx, ny, nz};
    p2p::quantise(J, res, o.a, &o.rho);
    o.partner = partner;
    return o;
}

// ---- the host's table: the same slots, filled one surfel after the other
struct SfgHostTable {
    const float *surfels;
    int count, slots, log2_slots;
    uint64_t *keys, *bids;  // [slots] each; the caller owns them
    uint64_t key(uint32_t slot) const { return keys[slot]; }
    uint64_t best(uint32_t slot) const { return bids[slot]; }
    SfgF4 quad(int r, int which) const {
        const float *s = surfels + (size_t)r * 12 + 4 * which;
        return SfgF4{s[0], s[1], s[2], s[3]};
    }
};

// TABLE: every in-grid surfel claims the slot of its voxel and bids for it. False when a walk visits every slot.
static inline bool sfg_fill_host(SfgHostTable *t, float inv) {
    for (int s = 0; s < t->slots; s++) {
        t->keys[s] = SFJ_EMPTY;
        t->bids[s] = 0;
    }
    const uint32_t mask = (uint32_t)t->slots - 1u;
    for (int e = 0; e < t->count; e++) {
        const float *s = t->surfels + (size_t)e * 12;
        uint64_t key = 0;
        if (!sfj_key_of(s[0], s[1], s[2], inv, &key)) continue;
        uint32_t slot = sfj_first_slot(key, t->log2_slots);
        int found = -1;
        for (int step = 0; step < t->slots; step++) {
            if (t->keys[slot] == SFJ_EMPTY) t->keys[slot] = key;
            if (t->keys[slot] == key) {
                found = (int)slot;
                break;
            }
            slot = (slot + 1u) & mask;
        }
        if (found < 0) return false;
        const uint64_t bid = sfj_candidate(sfj_rank_of(s[3]), (uint32_t)e);
        if (bid > t->bids[found]) t->bids[found] = bid;
    }
    return true;
}

// One linearisation over `count` source surfels at the estimate E: the 32 words, the counts and, where asked for, the pairs.
// False when a probe walk was lost.
template <class Table>
static inline bool sfg_linearise_host(const Table &t, const SfgRule &r, const float *E, const float *src, int count, long long *words, int *n_sampled,
                                      int *n_outside, int32_t *pairs) {
    for (int f = 0; f < SFG_SYSTEM_WORDS; f++) words[f] = 0;
    int sampled = 0, outside = 0;
    bool lost = false;
    for (int e = 0; e < count; e++) {
        const float *s = src + (size_t)e * 12;
        if (e % r.stride != 0 || !sfg_confident(r, s[3])) {
            if (pairs) pairs[e] = SFG_NOT_SAMPLED;
            continue;
        }
        sampled++;
        const SfgPair o = sfg_pair_core(t, r, E, SfgF4{s[0], s[1], s[2], s[3]}, SfgF4{s[8], s[9], s[10], s[11]});
        lost = lost || o.lost;
        if (o.outside) outside++;
        if (o.partner >= 0) p2p::accumulate(words, o.a, o.rho);
        if (pairs) pairs[e] = o.partner;
    }
    *n_sampled = sampled;
    *n_outside = outside;
    return !lost;
}
