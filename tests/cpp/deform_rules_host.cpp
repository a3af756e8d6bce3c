// The rules of the deformation graphs (staticfusion_amd/csrc/sf_deform_rules.h) and their solver (sf_deform_solve.h) on the
// host, under the address and undefined-behaviour sanitizers. The program replays the tables tests/test_deform_rules_cpu.py
// wrote from tests/deform_ref.py -- graphs, surfels with their expected bindings and deformed values, expected edges, poses,
// and solver cases with their expected transforms and energies -- and compares bit for bit, with guard words behind every
// output, which the functions must leave alone. The device runs the same text of the rules. Prints "ok <checks>".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../staticfusion_amd/csrc/sf_deform_rules.h"
#include "../../staticfusion_amd/csrc/sf_deform_solve.h"

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

static bool same(const float *a, const float *b, size_t n) {
    for (size_t i = 0; i < n; i++) {
        if (std::isnan(a[i]) && std::isnan(b[i])) continue;
        if (std::memcmp(a + i, b + i, 4) != 0) return false;
    }
    return true;
}

static const float GUARD = -5.f;
static bool guarded(const std::vector<float> &v, size_t used) {
    for (size_t i = used; i < v.size(); i++)
        if (v[i] != GUARD) return false;
    return true;
}

int main(int argc, char **argv) {
    if (argc != 2 || !(in = std::fopen(argv[1], "rb"))) {
        std::printf("usage: deform_rules_host <tables>\n");
        return 2;
    }
    const int n_tables = rd1<int32_t>();
    for (int t = 0; t < n_tables; t++) {
        const int G = rd1<int32_t>(), nq = rd1<int32_t>(), np = rd1<int32_t>();
        const float window = rd1<float>();
        const auto pos = rd<float>((size_t)3 * G), times = rd<float>((size_t)G), M = rd<float>((size_t)12 * G);
        const auto surf = rd<float>((size_t)12 * nq);
        const auto want_m = rd<int32_t>((size_t)nq), want_idx = rd<int32_t>((size_t)4 * nq);
        const auto want_w = rd<float>((size_t)4 * nq), want_s = rd<float>((size_t)12 * nq);
        const auto want_edges = rd<int32_t>((size_t)4 * G);
        const auto poses = rd<float>((size_t)16 * np), taus = rd<float>((size_t)np), want_poses = rd<float>((size_t)16 * np);
        for (int q = 0; q < nq; q++) {
            const float *s = surf.data() + (size_t)12 * q;
            int idx[4 + 4] = {0, 0, 0, 0, 77, 77, 77, 77};
            std::vector<float> w(4 + 8, GUARD), out(12 + 8, GUARD);
            const int m = sfd_bind_core(G, pos.data(), times.data(), window, s, s[6], -1, idx, w.data());
            CHECK(m == want_m[(size_t)q]);
            CHECK(std::memcmp(idx, want_idx.data() + (size_t)4 * q, 16) == 0 && idx[4] == 77 && idx[7] == 77);
            CHECK(same(w.data(), want_w.data() + (size_t)4 * q, 4) && guarded(w, 4));
            const int m2 = sfd_deform_surfel_core(G, pos.data(), times.data(), M.data(), window, s, out.data());
            CHECK(m2 == m);
            if (m2 == 0) {
                CHECK(guarded(out, 0));  // an unbound surfel: nothing is written
                CHECK(same(s, want_s.data() + (size_t)12 * q, 12));
            } else {
                CHECK(same(out.data(), want_s.data() + (size_t)12 * q, 12) && guarded(out, 12));
                std::vector<float> inplace(s, s + 12);  // out may be s
                sfd_deform_surfel_core(G, pos.data(), times.data(), M.data(), window, inplace.data(), inplace.data());
                CHECK(same(inplace.data(), out.data(), 12));
            }
        }
        for (int j = 0; j < G; j++) {
            int e4[4 + 2] = {0, 0, 0, 0, 77, 77};
            sfd_edges_core(G, pos.data(), times.data(), window, j, e4);
            CHECK(std::memcmp(e4, want_edges.data() + (size_t)4 * j, 16) == 0 && e4[4] == 77 && e4[5] == 77);
            for (int k = 0; k < 4; k++) CHECK(e4[k] != j && e4[k] >= -1 && e4[k] < G);
        }
        for (int q = 0; q < np; q++) {
            std::vector<float> out(16 + 8, GUARD);
            sfd_deform_pose_core(G, pos.data(), times.data(), M.data(), window, poses.data() + (size_t)16 * q, taus[(size_t)q], out.data());
            CHECK(same(out.data(), want_poses.data() + (size_t)16 * q, 16) && guarded(out, 16));
        }
    }
    const int n_solves = rd1<int32_t>();
    for (int t = 0; t < n_solves; t++) {
        const int G = rd1<int32_t>(), C = rd1<int32_t>(), iterations = rd1<int32_t>();
        const float window = rd1<float>(), w_reg = rd1<float>(), damping = rd1<float>();
        const auto pos = rd<float>((size_t)3 * G), times = rd<float>((size_t)G);
        auto M = rd<float>((size_t)12 * G);
        const auto cons = rd<float>((size_t)8 * C);
        const int want_status = rd1<int32_t>(), want_done = rd1<int32_t>(), want_bound = rd1<int32_t>();
        const auto want_energy = rd<double>(33);
        const auto want_M = rd<float>((size_t)12 * G);
        M.resize((size_t)12 * G + 8, GUARD);
        std::vector<double> energy(33 + 4, -5.0);
        for (int k = 0; k < 33; k++) energy[(size_t)k] = 0.0;
        int done = -1, bound = -1;
        static_assert(sizeof(SfdConstraint) == 32, "a constraint is eight floats");
        std::vector<SfdConstraint> cs((size_t)C);
        if (C) std::memcpy(cs.data(), cons.data(), (size_t)C * 32);
        const int status = sfd_solve_core(G, pos.data(), times.data(), C, cs.data(), window, w_reg, damping, iterations, M.data(), &done, &bound, energy.data());
        CHECK(status == want_status && done == want_done && bound == want_bound);
        CHECK(std::memcmp(energy.data(), want_energy.data(), 33 * 8) == 0 && energy[33] == -5.0 && energy[36] == -5.0);
        CHECK(same(M.data(), want_M.data(), (size_t)12 * G) && guarded(M, (size_t)12 * G));
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
