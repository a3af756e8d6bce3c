// sf_track_assign.h — the assignment of include/sf_tracks.h (step 3) that the host and the device share: which pairs are
// candidates, the total order they are walked in, and the greedy loop itself. Plain C++ on integers. The loop is written once
// for a TEAM of lanes: the host (sft_assign of sf_hip_tracks.hip, and tests/cpp/track_assign_host.cpp under the sanitizers) runs
// it with a team of one, the device (sft_assign_kernel of sf_tracks.h) with the lanes of one workgroup, so both run the same
// text and take the same pairs. It includes nothing of the library and defines no kernel.
//
// EVERY LOOP IS BOUNDED: at most min(k_prev, k) rounds, each one pass over the k_prev * k pairs and one team-wide maximum.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SFT_HD __host__ __device__
#else
#define SFT_HD
#endif

#define SFT_MAX_TRACKS 256  // the largest max_tracks of a tracker: t and k fit the 16-bit fields of a pair key

// A pair (t, k) of a previous track and a region, both 0-based here, with overlap o, n_prev pixels in the track and n_cur in
// the region: a candidate when o >= min_overlap and 1024 * o >= min_share * min(n_prev, n_cur), in int64.
SFT_HD static inline bool sft_candidate(int32_t o, int32_t n_prev, int32_t n_cur, int32_t min_overlap, int32_t min_share) {
    if (o < min_overlap) return false;
    const int64_t smaller = n_prev < n_cur ? n_prev : n_cur;
    return (int64_t)1024 * (int64_t)o >= (int64_t)min_share * smaller;
}

// The order of the walk as one number: a larger key is walked first. o descending, then t ascending, then k ascending; o >= 1
// for a candidate, so 0 is never a key.
SFT_HD static inline uint64_t sft_pair_key(int32_t o, int t, int k) {
    return ((uint64_t)(uint32_t)o << 32) | ((uint64_t)(0xFFFFu - (uint32_t)t) << 16) | (uint64_t)(0xFFFFu - (uint32_t)k);
}
SFT_HD static inline int sft_key_t(uint64_t key) { return (int)(0xFFFFu - (uint32_t)((key >> 16) & 0xFFFFu)); }
SFT_HD static inline int sft_key_k(uint64_t key) { return (int)(0xFFFFu - (uint32_t)(key & 0xFFFFu)); }

// A team of one: the host.
struct SftSolo {
    SFT_HD int lanes() const { return 1; }
    SFT_HD int lane() const { return 0; }
    SFT_HD void sync() const {}
    SFT_HD uint64_t max_of(uint64_t v) const { return v; }
};

// The greedy assignment. O is k_prev x k with row stride `stride` (O[t * stride + c]); n_prev holds k_prev counts, n_cur k.
// prev_of_cur (k entries) gets t + 1 of the track a region took, or 0; cur_of_prev (k_prev entries) c + 1 or 0. Both are
// written by the team and must be memory all its lanes see. Returns the number of pairs taken, which is the number of rounds
// that found a candidate; the loop ends at the first round that finds none, and never runs more than min(k_prev, k) rounds.
// Team: lanes(), lane(), sync() (a barrier that also orders the team's memory) and max_of(v) (every lane gets the largest v).
template <class Team>
SFT_HD static inline int sft_assign_rounds(const Team &team, int k_prev, int k, const int32_t *O, int stride, const int32_t *n_prev, const int32_t *n_cur,
                                           int32_t min_overlap, int32_t min_share, int32_t *prev_of_cur, int32_t *cur_of_prev) {
    const int lanes = team.lanes(), lane = team.lane();
    for (int c = lane; c < k; c += lanes) prev_of_cur[c] = 0;
    for (int t = lane; t < k_prev; t += lanes) cur_of_prev[t] = 0;
    team.sync();
    const int limit = k_prev < k ? k_prev : k;
    const int pairs = k_prev * k;  // <= 65536
    int taken = 0;
    for (int round = 0; round < limit; round++) {
        uint64_t best = 0;
        for (int p = lane; p < pairs; p += lanes) {
            const int t = p / k, c = p - t * k;
            if (cur_of_prev[t] != 0 || prev_of_cur[c] != 0) continue;
            const int32_t o = O[(int64_t)t * stride + c];
            if (!sft_candidate(o, n_prev[t], n_cur[c], min_overlap, min_share)) continue;
            const uint64_t key = sft_pair_key(o, t, c);
            if (key > best) best = key;
        }
        best = team.max_of(best);
        if (best == 0) break;  // (the whole team: max_of gives every lane the same value)
        const int t = sft_key_t(best), c = sft_key_k(best);
        if (lane == 0) {
            cur_of_prev[t] = c + 1;
            prev_of_cur[c] = t + 1;
        }
        taken++;
        team.sync();
    }
    return taken;
}
