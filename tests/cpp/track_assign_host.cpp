// The greedy assignment of the region tracks (staticfusion_amd/csrc/sf_track_assign.h) on the host, under the address and
// undefined-behaviour sanitizers: the hand tables of include/sf_tracks.h's step 3 (a split, a merge, equal overlaps, min_overlap
// and min_share at and below their bounds, empty tables, one track against 256 regions, a permutation of 256), every
// K_prev, K in {0, 1, 2, 255, 256} and 3000 random tables against a sort-and-walk statement of the same rule, and the number
// of rounds, counted by a team that counts its maxima: never more than min(K_prev, K). The device runs the same text.
// Prints "ok <checks>".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <tuple>
#include <vector>

#include "../../staticfusion_amd/csrc/sf_track_assign.h"

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

static uint64_t state = 88172645463325252ull;
static uint64_t next_u64() {
    state = 6364136223846793005ull * state + 1442695040888963407ull;
    return state >> 33;
}

// a team of one that counts the rounds: one maximum per round
struct Counting {
    mutable int maxima = 0;
    int lanes() const { return 1; }
    int lane() const { return 0; }
    void sync() const {}
    uint64_t max_of(uint64_t v) const {
        maxima++;
        return v;
    }
};

struct Result {
    std::vector<int32_t> prev_of_cur, cur_of_prev;
    int taken = 0, rounds = 0;
};

static Result run(int kp, int k, const std::vector<int32_t> &O, const std::vector<int32_t> &n_prev, const std::vector<int32_t> &n_cur, int min_overlap, int min_share) {
    Result r;
    r.prev_of_cur.assign((size_t)k + 1, -5);  // one past the end: a guard the loop must leave alone
    r.cur_of_prev.assign((size_t)kp + 1, -5);
    Counting team;
    r.taken = sft_assign_rounds(team, kp, k, O.data(), k, n_prev.data(), n_cur.data(), min_overlap, min_share, r.prev_of_cur.data(), r.cur_of_prev.data());
    r.rounds = team.maxima;
    CHECK(r.prev_of_cur[(size_t)k] == -5 && r.cur_of_prev[(size_t)kp] == -5);
    CHECK(r.rounds <= std::min(kp, k) && r.taken <= r.rounds && r.rounds <= r.taken + 1);
    const Result solo = [&] {
        Result s;
        s.prev_of_cur.assign((size_t)k + 1, -5);
        s.cur_of_prev.assign((size_t)kp + 1, -5);
        s.taken = sft_assign_rounds(SftSolo(), kp, k, O.data(), k, n_prev.data(), n_cur.data(), min_overlap, min_share, s.prev_of_cur.data(), s.cur_of_prev.data());
        return s;
    }();
    CHECK(solo.taken == r.taken && solo.prev_of_cur == r.prev_of_cur && solo.cur_of_prev == r.cur_of_prev);
    r.prev_of_cur.pop_back();
    r.cur_of_prev.pop_back();
    return r;
}

// the same rule, stated as a sort and a walk
static Result plain(int kp, int k, const std::vector<int32_t> &O, const std::vector<int32_t> &n_prev, const std::vector<int32_t> &n_cur, int min_overlap, int min_share) {
    std::vector<std::tuple<int64_t, int, int>> cand;
    for (int t = 0; t < kp; t++)
        for (int c = 0; c < k; c++) {
            const int64_t o = O[(size_t)t * k + c];
            if (o >= min_overlap && 1024 * o >= (int64_t)min_share * std::min<int64_t>(n_prev[(size_t)t], n_cur[(size_t)c])) cand.emplace_back(-o, t, c);
        }
    std::sort(cand.begin(), cand.end());
    Result r;
    r.prev_of_cur.assign((size_t)k, 0);
    r.cur_of_prev.assign((size_t)kp, 0);
    for (const auto &[neg, t, c] : cand) {
        (void)neg;
        if (r.cur_of_prev[(size_t)t] == 0 && r.prev_of_cur[(size_t)c] == 0) {
            r.cur_of_prev[(size_t)t] = c + 1;
            r.prev_of_cur[(size_t)c] = t + 1;
            r.taken++;
        }
    }
    return r;
}

static void both(int kp, int k, const std::vector<int32_t> &O, const std::vector<int32_t> &n_prev, const std::vector<int32_t> &n_cur, int min_overlap, int min_share) {
    const Result a = run(kp, k, O, n_prev, n_cur, min_overlap, min_share), b = plain(kp, k, O, n_prev, n_cur, min_overlap, min_share);
    CHECK(a.taken == b.taken && a.prev_of_cur == b.prev_of_cur && a.cur_of_prev == b.cur_of_prev);
}

typedef std::vector<int32_t> V;

int main() {
    // the order as one number
    CHECK(sft_pair_key(5, 0, 0) > sft_pair_key(4, 0, 0) && sft_pair_key(5, 0, 1) > sft_pair_key(5, 1, 0) && sft_pair_key(5, 1, 0) > sft_pair_key(5, 1, 1));
    CHECK(sft_pair_key(1, 255, 255) > 0 && sft_key_t(sft_pair_key(16777216, 255, 254)) == 255 && sft_key_k(sft_pair_key(16777216, 255, 254)) == 254);
    CHECK(sft_candidate(25, 100, 200, 1, 256) && !sft_candidate(24, 100, 200, 1, 256) && sft_candidate(25, 200, 100, 1, 256));
    CHECK(sft_candidate(4, 4, 4, 4, 256) && !sft_candidate(4, 4, 4, 5, 256) && sft_candidate(1, 100, 100, 1, 0) && !sft_candidate(99, 100, 100, 1, 1024));
    CHECK(sft_candidate(16777216, 16777216, 16777216, 1, 1024) && sft_candidate(2147483647, 2147483647, 2147483647, 2147483647, 1024));
    // a split: the larger overlap keeps the id
    Result r = run(1, 2, V{30, 50}, V{100}, V{35, 60}, 1, 256);
    CHECK(r.prev_of_cur == (V{0, 1}) && r.cur_of_prev == (V{2}) && r.taken == 1 && r.rounds == 1);
    // a merge
    r = run(2, 1, V{40, 25}, V{40, 25}, V{70}, 1, 256);
    CHECK(r.prev_of_cur == (V{1}) && r.cur_of_prev == (V{1, 0}) && r.taken == 1);
    // equal overlaps: t ascending, then k ascending
    r = run(2, 2, V{5, 5, 5, 5}, V{10, 10}, V{10, 10}, 1, 256);
    CHECK(r.prev_of_cur == (V{1, 2}) && r.cur_of_prev == (V{1, 2}) && r.taken == 2 && r.rounds == 2);
    r = run(2, 2, V{0, 5, 5, 5}, V{10, 10}, V{10, 10}, 1, 256);
    CHECK(r.prev_of_cur == (V{2, 1}) && r.cur_of_prev == (V{2, 1}));
    r = run(1, 3, V{5, 5, 5}, V{10}, V{10, 10, 10}, 1, 256);
    CHECK(r.prev_of_cur == (V{1, 0, 0}) && r.rounds == 1);
    // min_overlap met exactly and one below; min_share at equality and one pixel below
    CHECK(run(1, 1, V{4}, V{4}, V{4}, 4, 256).taken == 1 && run(1, 1, V{4}, V{4}, V{4}, 5, 256).taken == 0);
    CHECK(run(1, 1, V{25}, V{100}, V{200}, 1, 256).taken == 1 && run(1, 1, V{24}, V{100}, V{200}, 1, 256).taken == 0);
    // empty tables
    r = run(0, 3, V{}, V{}, V{7, 7, 7}, 1, 256);
    CHECK(r.prev_of_cur == (V{0, 0, 0}) && r.taken == 0 && r.rounds == 0);
    r = run(3, 0, V{}, V{7, 7, 7}, V{}, 1, 256);
    CHECK(r.cur_of_prev == (V{0, 0, 0}) && r.taken == 0 && r.rounds == 0);
    CHECK(run(0, 0, V{}, V{}, V{}, 1, 256).taken == 0 && run(2, 2, V{0, 0, 0, 0}, V{7, 7}, V{7, 7}, 1, 256).rounds == 1);
    // one track against 256 regions: the first of the largest
    {
        V row(256), n_cur(256, 1000);
        for (int c = 0; c < 256; c++) row[(size_t)c] = (c * 37) % 101 + 1;
        const int best = (int)(std::max_element(row.begin(), row.end()) - row.begin());
        r = run(1, 256, row, V{1000}, n_cur, 1, 0);
        CHECK(r.taken == 1 && r.rounds == 1 && r.cur_of_prev[0] == best + 1 && r.prev_of_cur[(size_t)best] == 1);
        r = run(256, 1, row, n_cur, V{1000}, 1, 0);  // and the other way round
        CHECK(r.taken == 1 && r.prev_of_cur[0] == best + 1);
    }
    // 256 against 256 with a permutation on the diagonal
    {
        V O((size_t)256 * 256, 0), n(256, 10);
        for (int t = 0; t < 256; t++) O[(size_t)t * 256 + (size_t)((t * 77 + 5) % 256)] = 10;
        r = run(256, 256, O, n, n, 1, 256);
        CHECK(r.taken == 256 && r.rounds == 256);
        for (int t = 0; t < 256; t++) CHECK(r.cur_of_prev[(size_t)t] == (t * 77 + 5) % 256 + 1 && r.prev_of_cur[(size_t)((t * 77 + 5) % 256)] == t + 1);
    }
    // every K_prev, K in {0, 1, 2, 255, 256}, dense random overlaps with many ties
    const int sizes[5] = {0, 1, 2, 255, 256};
    for (int kp : sizes)
        for (int k : sizes) {
            V O((size_t)kp * k), n_prev((size_t)kp), n_cur((size_t)k);
            for (auto &o : O) o = (int32_t)(next_u64() % 9);
            for (auto &x : n_prev) x = 1 + (int32_t)(next_u64() % 30);
            for (auto &x : n_cur) x = 1 + (int32_t)(next_u64() % 30);
            both(kp, k, O, n_prev, n_cur, 1 + (int)(next_u64() % 3), (int)(next_u64() % 1025));
        }
    // random small tables
    for (int i = 0; i < 3000; i++) {
        const int kp = (int)(next_u64() % 12), k = (int)(next_u64() % 12);
        V O((size_t)kp * k), n_prev((size_t)kp), n_cur((size_t)k);
        for (auto &o : O) o = (int32_t)(next_u64() % 6);
        for (auto &x : n_prev) x = 1 + (int32_t)(next_u64() % 24);
        for (auto &x : n_cur) x = 1 + (int32_t)(next_u64() % 24);
        both(kp, k, O, n_prev, n_cur, 1 + (int)(next_u64() % 3), (int)(next_u64() % 1025));
    }
    if (failures) return 1;
    std::printf("ok %lld\n", checked);
    return 0;
}
