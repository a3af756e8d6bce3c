// sf_join_key.h — the definitions of include/sf_join.h that the host and the device share: the voxel key of a position, the
// rank of a confidence, the size of a table, the first slot of a key and the transform of a merge. Plain C++, fp32 in the
// written order, one operation per expression (no contraction: -ffp-contract=off), so the host (sfj_voxel_key, sfj_hash_slot and
// sfj_table_slots of sf_hip_join.hip, and tests/cpp/join_key_host.cpp under the sanitizers) and the device (sf_voxel_table.h, sf_join.h) run
// the same text and give the same bits. It includes nothing of the library and defines no kernel.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SFJ_HD __host__ __device__
#else
#define SFJ_HD
#endif

#define SFJ_EMPTY (~0ull)            // never a key: the top bit of a key is clear
#define SFJ_Q_LIMIT 1048576.0f       // 2^20: a cell index q is in the grid when |q| < 2^20
#define SFJ_Q_BIAS 1048576           // q + 2^20 lies in 1 .. 2^21 - 1
#define SFJ_MIN_SLOTS 64
#define SFJ_MAX_COUNT (1 << 29)      // the largest count sfj_table_slots takes: 2^30 slots
#define SFJ_HASH_MUL 0x9E3779B97F4A7C15ull

SFJ_HD static inline bool sfj_finite(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return (u & 0x7f800000u) != 0x7f800000u;
}

// One coordinate: false when p or q = floorf(p * inv) is not finite or |q| >= 2^20; otherwise *cell_out = q + 2^20.
SFJ_HD static inline bool sfj_cell_index(float p, float inv, uint32_t *cell_out) {
    if (!sfj_finite(p)) return false;
    const float scaled = p * inv;
    const float q = floorf(scaled);
    if (!sfj_finite(q)) return false;
    if (!(fabsf(q) < SFJ_Q_LIMIT)) return false;
    *cell_out = (uint32_t)((int32_t)q + SFJ_Q_BIAS);  // q is an integer of magnitude < 2^20: the conversion is exact
    return true;
}

// The voxel key of (x, y, z) for inv = 1.0f / cell; false (and *key untouched) for a position outside the grid.
SFJ_HD static inline bool sfj_key_of(float x, float y, float z, float inv, uint64_t *key) {
    uint32_t cx = 0, cy = 0, cz = 0;
    if (!sfj_cell_index(x, inv, &cx)) return false;
    if (!sfj_cell_index(y, inv, &cy)) return false;
    if (!sfj_cell_index(z, inv, &cz)) return false;
    *key = ((uint64_t)cx << 42) | ((uint64_t)cy << 21) | (uint64_t)cz;
    return true;
}

// The rank of a confidence: NaN 0, a set sign ~bits, otherwise bits | 0x80000000. It orders like the numbers, -0 below +0, a
// NaN below every number.
SFJ_HD static inline uint32_t sfj_rank_of(float confidence) {
    uint32_t u;
    memcpy(&u, &confidence, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// what atomicMax decides a voxel by: the higher rank, then the lower index
SFJ_HD static inline uint64_t sfj_candidate(uint32_t rank, uint32_t index) { return ((uint64_t)rank << 32) | (uint64_t)(0xFFFFFFFFu - index); }

// The smallest power of two >= max(2 * count, 64); count in 0 .. SFJ_MAX_COUNT (the caller checks).
SFJ_HD static inline int sfj_slots_for(int count) {
    const int64_t want = 2 * (int64_t)count;
    int64_t slots = SFJ_MIN_SLOTS;
    while (slots < want) slots *= 2;
    return (int)slots;
}

SFJ_HD static inline int sfj_log2_of(int slots) {  // slots: a power of two
    int l = 0;
    while ((1 << l) < slots) l++;
    return l;
}

// The first slot of a key in a table of 2^log2_slots slots (log2_slots in 6 .. 30).
SFJ_HD static inline uint32_t sfj_first_slot(uint64_t key, int log2_slots) { return (uint32_t)((key * SFJ_HASH_MUL) >> (64 - log2_slots)); }

// Row r of the merge's transform, T 4 x 4 column-major: ((T[r] * x + T[4 + r] * y) + T[8 + r] * z) + w * T[12 + r], the last
// term added for a position (translate) and left out for a normal.
SFJ_HD static inline float sfj_transform_row(const float *T, int r, float x, float y, float z, bool translate) {
    const float a = T[r] * x;
    const float b = T[4 + r] * y;
    const float c = T[8 + r] * z;
    const float ab = a + b;
    const float abc = ab + c;
    return translate ? abc + T[12 + r] : abc;
}
