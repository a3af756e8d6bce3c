// The rules SAMPLE, PAIR and the row of the map registration (staticfusion_amd/csrc/sf_register_rules.h) and the step it shares
// with the pose refinement (sf_align_step.h) on the host, under the address and undefined-behaviour sanitizers. The program
// replays the table tests/test_register_rules_cpu.py wrote from tests/register_ref.py -- destination and source surfels, the
// parameters, the estimate, and the expected 32 words, counts and pairs -- and compares exactly; then the loops the table holds,
// linearise and step in turn, against the expected estimates bit for bit. The surfels, the table's slots and the pairs lie in heap
// blocks of exactly their size (the sanitizer sees a read or write beyond them), and the pairs have guard words around them. The
// device runs the same text. Before the table, quantise and accumulate of sf_p2p_system.h are called directly on the edge values of
// the row and on 10 000 random rows, against the expressions written out here. Prints "ok <checks>".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../staticfusion_amd/csrc/sf_align_step.h"
#include "../../staticfusion_amd/csrc/sf_register_rules.h"

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

struct Case {
    std::vector<float> dst, src;
    std::vector<uint64_t> keys, bids;
    SfgHostTable t;
    SfgRule rule;
};

// dst_count, src_count, then the surfels; cell, dist_max, min_cos, min_confidence; stride
static void read_case(Case &c) {
    const int nd = rd1<int32_t>(), ns = rd1<int32_t>();
    c.dst = rd<float>((size_t)nd * 12);
    c.src = rd<float>((size_t)ns * 12);
    const auto pf = rd<float>(4);
    const int stride = rd1<int32_t>();
    c.rule = SfgRule{1.0f / pf[0], pf[1], pf[2], pf[3], pf[3] > 0.f, stride};
    c.t.surfels = c.dst.data();
    c.t.count = nd;
    c.t.slots = sfj_slots_for(nd);
    c.t.log2_slots = sfj_log2_of(c.t.slots);
    c.keys.assign((size_t)c.t.slots, 0);
    c.bids.assign((size_t)c.t.slots, 0);
    c.t.keys = c.keys.data();
    c.t.bids = c.bids.data();
    CHECK(sfg_fill_host(&c.t, c.rule.inv));
}

static void linearise(const Case &c, const double *E, const int64_t *want, int want_sampled, int want_outside, const int32_t *want_pairs) {
    const int GUARD = -77;
    const int ns = (int)(c.src.size() / 12);
    float Ef[12];
    for (int k = 0; k < 12; k++) Ef[k] = (float)E[k];
    long long w[SFG_SYSTEM_WORDS];
    int n_sampled = -1, n_outside = -1;
    std::vector<int32_t> pairs((size_t)ns + 2, GUARD);  // guard, the pairs, guard
    CHECK(sfg_linearise_host(c.t, c.rule, Ef, c.src.data(), ns, w, &n_sampled, &n_outside, pairs.data() + 1));
    for (int f = 0; f < SFG_SYSTEM_WORDS; f++) CHECK((int64_t)w[f] == want[f]);
    CHECK(n_sampled == want_sampled && n_outside == want_outside);
    if (want_pairs)
        for (int e = 0; e < ns; e++) CHECK(pairs[(size_t)e + 1] == want_pairs[e]);
    CHECK(pairs[0] == GUARD && pairs[(size_t)ns + 1] == GUARD);
    // without room for the pairs the sums are the same
    long long w2[SFG_SYSTEM_WORDS];
    CHECK(sfg_linearise_host(c.t, c.rule, Ef, c.src.data(), ns, w2, &n_sampled, &n_outside, nullptr));
    CHECK(std::memcmp(w, w2, sizeof(w)) == 0);
}

// quantise and accumulate of sf_p2p_system.h against the expressions written out here: the row J and the residual r
static void system_row(const float J[6], float r) {
    int a[6] = {7, 7, 7, 7, 7, 7}, rho = 7;
    p2p::quantise(J, r, a, &rho);
    for (int k = 0; k < 6; k++) CHECK(a[k] == (int)rintf(fminf(fmaxf(J[k], -64.f), 64.f) * 4096.f) && std::abs(a[k]) <= 1 << 18);
    CHECK(rho == (int)rintf(r * 65536.f));
    long long acc[p2p::WORDS], want[p2p::WORDS];
    for (int f = 0; f < p2p::WORDS; f++) acc[f] = want[f] = 1000 + f;
    for (int twice = 0; twice < 2; twice++) {
        p2p::accumulate(acc, a, rho);
        want[0] += 1;
        want[1] += (long long)rho * rho;
        int f = 8;
        for (int k = 0; k < 6; k++) {
            want[2 + k] += (long long)a[k] * rho;
            for (int l = k; l < 6; l++) want[f++] += (long long)a[k] * a[l];
        }
        CHECK(f == p2p::FIELDS);
    }
    CHECK(std::memcmp(acc, want, sizeof(acc)) == 0);  // (the three reserved words are not touched)
}

static void system_rows() {
    static_assert(p2p::FIELDS == 29 && p2p::WORDS == 32, "n, ss, g[6], H[21] and three reserved words");
    // the edge values: +-64 exactly, beyond, +-0, NaN, and with them the largest r that dist_max <= 1 admits
    const float edge[12] = {64.f, -64.f, 64.000008f, -64.000008f, 1e30f, -1e30f, INFINITY, -INFINITY, 0.f, -0.f, NAN, 63.999996f};
    const float res[6] = {1.f, -1.f, 0.f, -0.f, 0.99999994f, 7.6293945e-06f};
    for (int s = 0; s < 12; s++) {
        float J[6];
        for (int k = 0; k < 6; k++) J[k] = edge[(s + 5 * k) % 12];
        system_row(J, res[s % 6]);
    }
    const float nan6[6] = {NAN, NAN, NAN, NAN, NAN, NAN};
    int a[6], rho;
    p2p::quantise(nan6, 1.f, a, &rho);
    for (int k = 0; k < 6; k++) CHECK(a[k] == -64 * 4096);  // fmaxf returns the bound
    CHECK(rho == 65536);
    uint64_t state = 0x9E3779B97F4A7C15ull;  // 10 000 random rows: J in [-80, 80), a third of them in [-1, 1); r in [-1, 1)
    const auto uniform = [&state]() {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        return (float)(state >> 40) * (1.0f / 8388608.0f) - 1.0f;
    };
    for (int t = 0; t < 10000; t++) {
        float J[6];
        for (int k = 0; k < 6; k++) J[k] = uniform() * ((t + k) % 3 ? 80.f : 1.f);
        system_row(J, uniform());
    }
}

int main(int argc, char **argv) {
    if (argc != 2 || !(in = std::fopen(argv[1], "rb"))) {
        std::printf("usage: register_rules_host <table>\n");
        return 2;
    }
    system_rows();
    const int n_cases = rd1<int32_t>();
    for (int t = 0; t < n_cases; t++) {
        Case c;
        read_case(c);
        const int ns = (int)(c.src.size() / 12);
        const auto E = rd<double>(12);
        const auto want = rd<int64_t>(SFG_SYSTEM_WORDS);
        const auto counts = rd<int32_t>(2);
        const auto pairs = rd<int32_t>((size_t)ns);
        linearise(c, E.data(), want.data(), counts[0], counts[1], pairs.data());
    }
    // loops: the case, E0, damping, the number of steps, then per step the expected words and the expected estimate after it
    const int n_loops = rd1<int32_t>();
    for (int t = 0; t < n_loops; t++) {
        Case c;
        read_case(c);
        auto E = rd<double>(12);
        const float damping = rd1<float>();
        const int steps = rd1<int32_t>();
        for (int it = 0; it < steps; it++) {
            const auto want = rd<int64_t>(SFG_SYSTEM_WORDS);
            const auto counts = rd<int32_t>(2);
            const auto status = rd1<int32_t>();
            const auto E_want = rd<double>(12);
            linearise(c, E.data(), want.data(), counts[0], counts[1], nullptr);
            double En[12];
            const int got = sfa_step_core(want.data(), damping, E.data(), En);
            CHECK(got == status);
            if (got == SFA_STEP_OK) {
                CHECK(std::memcmp(En, E_want.data(), sizeof(En)) == 0);
                std::memcpy(E.data(), En, sizeof(En));
            }
        }
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
