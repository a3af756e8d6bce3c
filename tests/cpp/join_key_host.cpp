// The key, the rank, the hash and the table size of the joined maps (staticfusion_amd/csrc/sf_join_key.h) on the host, under
// the address and undefined-behaviour sanitizers: the hand-computed key, cell borders, |q| = 2^20 - 1 and 2^20 on every axis and
// side (the float-to-int conversion runs only inside the grid), NaN, +-inf, -0.0, a cell so small that p * inv overflows, keys
// at both ends of the range against ~0, the ranks of the special confidences in their order, the first slot for every table
// size with the shifts at their limits, the table sizes up to 2^29 surfels, the transform rows, and 200 000 random positions
// whose keys decode back to floor(p * inv). The device runs the same text. Prints "ok <checks>".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../../staticfusion_amd/csrc/sf_join_key.h"

static long long checked = 0;
static int failures = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        checked++;                                                    \
        if (!(cond)) {                                                \
            std::printf("FAIL line %d: %s\n", __LINE__, #cond);       \
            failures++;                                               \
        }                                                             \
    } while (0)

static uint64_t key_of(int64_t qx, int64_t qy, int64_t qz) {
    const int64_t b = 1 << 20;
    return ((uint64_t)(qx + b) << 42) | ((uint64_t)(qy + b) << 21) | (uint64_t)(qz + b);
}

static uint64_t state = 88172645463325252ull;
static uint64_t next_u64() {
    state = 6364136223846793005ull * state + 1442695040888963407ull;
    return state;
}
static float uniform(float lo, float hi) { return lo + (hi - lo) * (float)((double)(next_u64() >> 11) / 9007199254740992.0); }

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    uint64_t key = 77;
    // ---- by hand, -0.0, borders
    const float inv = 1.0f / 0.02f;
    CHECK(sfj_key_of(0.03f, -0.01f, 0.0f, inv, &key) && key == key_of(1, -1, 0));
    CHECK(sfj_key_of(-0.0f, 0.0f, -0.0f, inv, &key) && key == key_of(0, 0, 0));
    for (int k = -1000; k <= 1000; k++) {
        CHECK(sfj_key_of(0.25f * (float)k, 0.0f, 0.0f, 4.0f, &key) && key == key_of(k, 0, 0));
        CHECK(sfj_key_of(std::nextafterf(0.25f * (float)k, -1e9f), 0.0f, 0.0f, 4.0f, &key) && key == key_of(k - 1, 0, 0));
    }
    // ---- the ends of the grid at cell 1, every axis and side; both ends of the key range
    const float last = 1048575.0f, limit = 1048576.0f;
    for (int axis = 0; axis < 3; axis++)
        for (int side = -1; side <= 1; side += 2) {
            float p[3] = {0.5f, 0.5f, 0.5f};
            int64_t q[3] = {0, 0, 0};
            p[axis] = (float)side * last;
            q[axis] = side * 1048575;
            CHECK(sfj_key_of(p[0], p[1], p[2], 1.0f, &key) && key == key_of(q[0], q[1], q[2]));
            key = 77;
            p[axis] = (float)side * limit;
            CHECK(!sfj_key_of(p[0], p[1], p[2], 1.0f, &key) && key == 77);
            p[axis] = (float)side * 3e9f;  // beyond int32: never converted
            CHECK(!sfj_key_of(p[0], p[1], p[2], 1.0f, &key) && key == 77);
            p[axis] = (float)side * 3.4e38f;
            CHECK(!sfj_key_of(p[0], p[1], p[2], 1.0f, &key) && key == 77);
        }
    CHECK(sfj_key_of(last + 0.5f, 0.f, 0.f, 1.0f, &key) && key == key_of(1048575, 0, 0));
    key = 77;
    CHECK(!sfj_key_of(-last - 0.5f, 0.f, 0.f, 1.0f, &key) && key == 77);
    CHECK(sfj_key_of(last, last, last, 1.0f, &key) && key == key_of(1048575, 1048575, 1048575) && key < (1ull << 63) && key != SFJ_EMPTY);
    CHECK(sfj_key_of(-last, -last, -last, 1.0f, &key) && key == key_of(-1048575, -1048575, -1048575) && key == ((1ull << 42) | (1ull << 21) | 1ull));
    // ---- NaN, +-inf, overflow of p * inv
    key = 77;
    const float bad[3] = {nan, inf, -inf};
    for (float b : bad)
        for (int axis = 0; axis < 3; axis++) {
            float p[3] = {0.01f, 0.01f, 0.01f};
            p[axis] = b;
            CHECK(!sfj_key_of(p[0], p[1], p[2], inv, &key) && key == 77);
        }
    const float huge_inv = 1.0f / 1.17549435e-38f;  // 2^126
    CHECK(std::isfinite(huge_inv));
    CHECK(!sfj_key_of(8.0f, 0.f, 0.f, huge_inv, &key) && !sfj_key_of(0.f, -8.0f, 0.f, huge_inv, &key) && !sfj_key_of(0.f, 0.f, 1.0f, huge_inv, &key) && key == 77);
    CHECK(sfj_key_of(0.f, 0.f, 0.f, huge_inv, &key) && key == key_of(0, 0, 0));
    // ---- ranks
    const float neg_nan = std::copysign(nan, -1.0f);
    CHECK(sfj_rank_of(nan) == 0u && sfj_rank_of(neg_nan) == 0u);
    CHECK(sfj_rank_of(-1.0f) == 0x407FFFFFu && sfj_rank_of(-0.0f) == 0x7FFFFFFFu && sfj_rank_of(0.0f) == 0x80000000u && sfj_rank_of(1.0f) == 0xBF800000u);
    const float tiny = std::numeric_limits<float>::denorm_min();
    const float order[] = {-inf, -3e38f, -1.0f, -tiny, -0.0f, 0.0f, tiny, 0.08f, 1.0f, 3e38f, inf};
    for (size_t k = 0; k + 1 < sizeof order / sizeof order[0]; k++) CHECK(sfj_rank_of(order[k]) < sfj_rank_of(order[k + 1]) && sfj_rank_of(order[k]) > 0u);
    CHECK(sfj_candidate(5u, 0u) > sfj_candidate(5u, 1u) && sfj_candidate(6u, 0xFFFFFFFEu) > sfj_candidate(5u, 0u) && sfj_candidate(0u, 0xFFFFFFFEu) > 0ull);
    // ---- table sizes and first slots
    CHECK(sfj_slots_for(0) == 64 && sfj_slots_for(32) == 64 && sfj_slots_for(33) == 128 && sfj_slots_for(262144) == 524288 && sfj_slots_for(262145) == 1048576);
    CHECK(sfj_slots_for(SFJ_MAX_COUNT) == (1 << 30) && sfj_slots_for(SFJ_MAX_COUNT - 1) == (1 << 30) && sfj_slots_for((1 << 28) + 1) == (1 << 30));
    for (int l = 6; l <= 30; l++) {
        CHECK(sfj_log2_of(1 << l) == l);
        const uint64_t keys[] = {0ull, 1ull, ~0ull, ~0ull - 1, 1ull << 63, key_of(0, 0, 0), key_of(1048575, 1048575, 1048575)};
        for (uint64_t k : keys) {
            const uint32_t slot = sfj_first_slot(k, l);
            CHECK(slot < (1u << l) && slot == (uint32_t)((unsigned __int128)k * SFJ_HASH_MUL % ((unsigned __int128)1 << 64) >> (64 - l)));
        }
    }
    // ---- the transform rows: the identity leaves finite values as they are, a normal gets no translation
    const float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    const float T[16] = {0, 1, 0, 0, -1, 0, 0, 0, 0, 0, 1, 0, 0.5f, -2.0f, 3.0f, 1};  // a quarter turn about z, then a shift
    CHECK(sfj_transform_row(I, 0, 1.5f, -2.5f, 3.5f, true) == 1.5f && sfj_transform_row(I, 1, 1.5f, -2.5f, 3.5f, true) == -2.5f);
    CHECK(sfj_transform_row(T, 0, 1.0f, 2.0f, 3.0f, true) == -1.5f && sfj_transform_row(T, 1, 1.0f, 2.0f, 3.0f, true) == -1.0f);
    CHECK(sfj_transform_row(T, 2, 1.0f, 2.0f, 3.0f, true) == 6.0f && sfj_transform_row(T, 0, 1.0f, 2.0f, 3.0f, false) == -2.0f);
    CHECK(std::isnan(sfj_transform_row(I, 0, 1.0f, inf, 0.0f, true)));  // 0 * inf
    // ---- random positions: the key decodes to floor(p * inv), or the position is outside for the stated reason
    const float cells[] = {0.02f, 0.01f, 0.05f, 1e-5f, 7.0f};
    for (int t = 0; t < 200000; t++) {
        const float c = cells[t % 5], ci = 1.0f / c;
        const float p[3] = {uniform(-40.f, 40.f), uniform(-40.f, 40.f), uniform(-40.f, 40.f)};
        bool in = true;
        int64_t q[3];
        for (int i = 0; i < 3; i++) {
            const float f = std::floor(p[i] * ci);
            in = in && std::fabs(f) < 1048576.0f;
            q[i] = in ? (int64_t)f : 0;
        }
        key = 77;
        const bool got = sfj_key_of(p[0], p[1], p[2], ci, &key);
        CHECK(got == in && key == (in ? key_of(q[0], q[1], q[2]) : 77ull));
    }
    if (failures) return 1;
    std::printf("ok %lld\n", checked);
    return 0;
}
