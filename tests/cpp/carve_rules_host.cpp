// The rules OBSERVE and DECIDE of the carve (staticfusion_amd/csrc/sf_carve_rules.h) on the host, under the address and
// undefined-behaviour sanitizers. The program replays the table tests/test_carve_rules_cpu.py wrote from tests/carve_ref.py --
// surfels with their view, parameters and depth frame and the expected class and counts, then votes with the expected decision
// -- and compares exactly. The surfel, the frame and the three counts lie in heap blocks of exactly their size (the sanitizer
// sees a read or write beyond them), and the counts have guard words around them. The device runs the same text. Prints
// "ok <checks>".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../staticfusion_amd/csrc/sf_carve_rules.h"

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

int main(int argc, char **argv) {
    if (argc != 2 || !(in = std::fopen(argv[1], "rb"))) {
        std::printf("usage: carve_rules_host <table>\n");
        return 2;
    }
    const int GUARD = -77;
    const int n_rows = rd1<int32_t>();
    for (int t = 0; t < n_rows; t++) {
        const auto s = rd<float>(12), T = rd<float>(16), f = rd<float>(8);
        const auto vi = rd<int32_t>(3);
        const auto pf = rd<float>(4);
        const auto pi = rd<int32_t>(4);
        SfeView v;
        std::memcpy(v.t_inv, T.data(), sizeof(v.t_inv));
        v.cx = f[0]; v.cy = f[1]; v.fx = f[2]; v.fy = f[3];
        v.max_depth = f[4]; v.min_confidence = f[5]; v.tick = f[6]; v.max_age = f[7];
        v.use_age = vi[0]; v.rows = vi[1]; v.cols = vi[2];
        const SfeRule r{pf[0], pf[1], pf[2], pf[3], pi[0], pi[1], pi[2], pi[3]};
        const auto zf = rd<float>((size_t)v.rows * v.cols);
        const auto want = rd<int32_t>(4);  // class, through, near, front
        std::vector<int> out(5, GUARD);    // guard, the three counts, guard
        const int cls = sfe_observe_core(s.data(), &v, zf.data(), &r, out.data() + 1);
        CHECK(cls == want[0]);
        CHECK(out[1] == want[1] && out[2] == want[2] && out[3] == want[3]);
        CHECK(out[0] == GUARD && out[4] == GUARD);
    }
    const int n_votes = rd1<int32_t>();
    for (int t = 0; t < n_votes; t++) {
        const auto d = rd<int32_t>(5);
        const SfeRule r{0.f, 0.f, 1.f, 0.f, 0, 1, d[2], d[3]};
        CHECK((sfe_decide_core(d[0], d[1], &r) ? 1 : 0) == d[4]);
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
