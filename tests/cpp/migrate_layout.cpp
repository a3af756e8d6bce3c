// The pure-host arithmetic of stream migration (staticfusion_amd/csrc/sf_migrate_layout.h): blob layout and ring rotation.
// Stand-alone: no HIP runtime, no library. tests/test_stream_migration_abi.py compiles it with -fsanitize=address,undefined
// and runs it as a child process; it prints "ok <checks>" and returns 0, or names the first failure and returns 1.
#include <cstdio>
#include <cstring>
#include <set>

#include "../../staticfusion_amd/csrc/sf_migrate_layout.h"

static long checks = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        checks++;                                                       \
        if (!(cond)) {                                                  \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                   \
        }                                                               \
    } while (0)

int main() {
    // ---- the ring: for every pair of counts 0..12 the five ages map source slots onto destination slots one to one
    for (int s = 0; s <= 12; s++)
        for (int d = 0; d <= 12; d++) {
            std::set<int> from, to;
            for (int a = 0; a < SF_HISTORY; a++) {
                const int fs = sfm_ring_slot(s, a), ts = sfm_ring_slot(d, a);
                CHECK(fs >= 0 && fs < SF_HISTORY && ts >= 0 && ts < SF_HISTORY);
                from.insert(fs);
                to.insert(ts);
            }
            CHECK(from.size() == (size_t)SF_HISTORY && to.size() == (size_t)SF_HISTORY);
            // equal or both mature, and nothing else
            CHECK(sfm_counts_compatible(s, d) == (s == d || (s >= SF_HISTORY && d >= SF_HISTORY)));
        }
    for (int c = 0; c <= 12; c++) {
        CHECK(sfm_ring_slot(c, 0) == c % SF_HISTORY);  // age 0 is the slot frame c overwrites (ring[im_count % 5] = current)
        // played through: frames 0 .. c - 1 each wrote ring[f % 5] = f; the entry of age a is then the one frame c - 5 + a wrote
        int ring[SF_HISTORY];
        for (int q = 0; q < SF_HISTORY; q++) ring[q] = -1 - q;  // (never written: distinct marks)
        for (int f = 0; f < c; f++) ring[f % SF_HISTORY] = f;
        for (int a = 0; a < SF_HISTORY; a++)
            if (c - SF_HISTORY + a >= 0) CHECK(ring[sfm_ring_slot(c, a)] == c - SF_HISTORY + a);
        // moved to a handle at count d and played on there: frame d + a of the destination overwrites what was age a
        for (int d = 0; d <= 12; d++) {
            int moved[SF_HISTORY];
            for (int a = 0; a < SF_HISTORY; a++) moved[sfm_ring_slot(d, a)] = ring[sfm_ring_slot(c, a)];
            for (int a = 0; a < SF_HISTORY; a++) CHECK(moved[(d + a) % SF_HISTORY] == ring[(c + a) % SF_HISTORY]);
        }
    }
    CHECK(!sfm_counts_compatible(-1, -1) && !sfm_counts_compatible(3, 9) && !sfm_counts_compatible(9, 3) && sfm_counts_compatible(7, 9));

    // ---- the layout: offsets increase, every segment starts on a multiple of 16 and the last one ends at the total
    const int geo[][4] = {{60, 80, 3, 0}, {60, 80, 3, 1}, {40, 42, 3, 0}, {40, 42, 3, 1}, {18, 22, 1, 0}, {18, 22, 1, 1}, {240, 320, 5, 1}, {8, 8, 1, 0}};
    for (const auto &g : geo) {
        SfmLayout lay;
        std::memset(&lay, 0xee, sizeof(lay));
        CHECK(sfm_layout(g[0], g[1], g[2], g[3], &lay));
        CHECK(lay.n0 == (size_t)g[0] * g[1]);
        size_t tot = 0;
        for (int L = 0; L < g[2]; L++) tot += (size_t)(g[0] >> L) * (g[1] >> L);
        CHECK(lay.n_tot == tot);
        CHECK(lay.segments == (g[3] ? SFM_SEG_COUNT : SFM_SEG_COUNT_NO_INPUT));
        CHECK(lay.offset[0] == SFM_HEADER_BYTES);
        size_t sum = SFM_HEADER_BYTES;
        for (int q = 0; q < lay.segments; q++) {
            CHECK(lay.offset[q] % 16 == 0);
            CHECK(lay.bytes[q] > 0 && lay.bytes[q] == sfm_segment_bytes(q, lay.n0, lay.n_tot));
            CHECK(lay.offset[q + 1] > lay.offset[q]);
            CHECK(lay.offset[q + 1] >= lay.offset[q] + lay.bytes[q] && lay.offset[q + 1] - lay.offset[q] - lay.bytes[q] < 16);
            sum += sfm_pad16(lay.bytes[q]);
        }
        CHECK(lay.offset[lay.segments] == lay.total && sum == lay.total && lay.offset[SFM_SEG_COUNT] == lay.total);
        // the blob without input images is a prefix of the one with them
        SfmLayout other;
        CHECK(sfm_layout(g[0], g[1], g[2], !g[3], &other));
        for (int q = 0; q < SFM_SEG_COUNT_NO_INPUT; q++) CHECK(other.offset[q] == lay.offset[q] && other.bytes[q] == lay.bytes[q]);
    }
    SfmLayout lay;
    CHECK(!sfm_layout(4, 4, 1, 0, &lay) && !sfm_layout(60, 80, 0, 0, &lay) && !sfm_layout(60, 80, 9, 0, &lay) && !sfm_layout(16, 16, 4, 0, &lay));
    CHECK(sizeof(SfmHeader) == SFM_HEADER_BYTES);
    CHECK(sfm_pad16(0) == 0 && sfm_pad16(1) == 16 && sfm_pad16(16) == 16 && sfm_pad16(6300) == 6304);
    std::printf("ok %ld\n", checks);
    return 0;
}
