// The PER SAMPLE rule of the closure constraints (staticfusion_amd/csrc/sf_closure_rules.h) on the host, under the address and
// undefined-behaviour sanitizers. The program replays the table tests/test_closure_rules_cpu.py wrote from tests/closure_ref.py
// -- samples with their expected mask, sum terms and records, then sample counts along an axis -- and compares bit for bit,
// with guard words around the two records, which the function must leave alone unless it sets their bits. The device runs the
// same text. Prints "ok <checks>".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../staticfusion_amd/csrc/sf_closure_rules.h"

static long long checked = 0;
static int failures = 0;
#define CHECK(cond)                                                           \
    do {                                                                      \
        checked++;                                                            \
        if (!(cond)) {                                                        \
            if (failures < 20) std::printf("FAIL line %d: %s\n", __LINE__, #cond); \
            failures++;                                                       \
        }                                                                     \
    } while (0)

static FILE *in = nullptr;
template <class T>
static std::vector<T> rd(size_t n) {
    std::vector<T> v(n);
    if (n && std::fread(v.data(), sizeof(T), n, in) != n) {
        std::printf("FAIL: the table file ends early\n");
        std::exit(2);
    }
    return v;
}
template <class T>
static T rd1() {
    return rd<T>(1)[0];
}

static const float GUARD = -5.f;
static void fill_guard(SfcRecord &r) {
    float f[8];
    for (int i = 0; i < 8; i++) f[i] = GUARD;
    std::memcpy(&r, f, sizeof(r));
}
static bool guarded(const SfcRecord &r) {
    float f[8];
    std::memcpy(f, &r, sizeof(r));
    for (int i = 0; i < 8; i++)
        if (f[i] != GUARD) return false;
    return true;
}

int main(int argc, char **argv) {
    if (argc != 2 || !(in = std::fopen(argv[1], "rb"))) {
        std::printf("usage: closure_rules_host <table>\n");
        return 2;
    }
    static_assert(sizeof(SfcRecord) == 32, "a record is eight floats");
    const int n_rows = rd1<int32_t>();
    for (int t = 0; t < n_rows; t++) {
        const int has_a = rd1<int32_t>(), has_o = rd1<int32_t>(), pins = rd1<int32_t>();
        const auto f = rd<float>(7);
        // exactly eight floats per surfel, as the kernel gathers them: the rule reads no more (the sanitizer would see it)
        const auto sa = rd<float>(8), so = rd<float>(8), T = rd<float>(16), P = rd<float>(16);
        const int want_mask = rd1<int32_t>();
        const long long want_dz = rd1<int64_t>(), want_shift = rd1<int64_t>();
        const int want_n = rd1<int32_t>();
        const auto want = rd<SfcRecord>((size_t)want_n);
        const SfcRule rule{pins, f[2], f[3], f[4], f[5], f[6]};
        std::vector<SfcRecord> out(4);  // guard, link, pin, guard
        for (auto &r : out) fill_guard(r);
        long long q_dz = -1, q_shift = -1;
        const int mask = sfc_link_core(has_a != 0, has_a ? sa.data() : nullptr, has_o != 0, has_o ? so.data() : nullptr, f[0], f[1], T.data(), P.data(), &rule,
                                       &out[1], &out[2], &q_dz, &q_shift);
        CHECK(mask == want_mask);
        CHECK(q_dz == want_dz && q_shift == want_shift);
        CHECK(guarded(out[0]) && guarded(out[3]));
        CHECK((mask & SFC_BIT_LINK) || guarded(out[1]));
        CHECK((mask & SFC_BIT_PIN) || guarded(out[2]));
        int k = 0;
        if (mask & SFC_BIT_LINK) {
            CHECK(k < want_n && std::memcmp(&out[1], &want[(size_t)k], 32) == 0);
            k++;
        }
        if (mask & SFC_BIT_PIN) {
            CHECK(k < want_n && std::memcmp(&out[2], &want[(size_t)k], 32) == 0);
            k++;
        }
        CHECK(k == want_n);
    }
    for (int t = 0; t < 10; t++) {
        const int extent = rd1<int32_t>(), stride = rd1<int32_t>(), want = rd1<int32_t>();
        CHECK(sfc_samples_along(extent, stride) == want);
    }
    unsigned char tail;
    CHECK(std::fread(&tail, 1, 1, in) == 0);  // the whole file has been replayed
    std::fclose(in);
    if (failures) {
        std::printf("%d of %lld checks failed\n", failures, checked);
        return 1;
    }
    std::printf("ok %lld\n", checked);
    return 0;
}
