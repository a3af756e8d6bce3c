// The index arithmetic of the region kernels (staticfusion_amd/csrc/sf_region_walk.h) held to the plain divisions it replaces,
// on the host. For every geometry below: the tiles cover every pixel exactly once; the border items are exactly the pixels
// of the first row of every tile row but the first and of the first column of every tile column but the first, each inside
// the image with its row v - 1 (column u - 1) inside too; every pair of 8-neighbours that lie in different tiles is reached
// from some item by the pairs sfr_border_kernel forms; and a lane's (v, u) counters equal i % rows and i / rows for its
// SFR_RUN indices, which never leave the entry's stride. Every address the kernels form comes from these values, so this is
// the bounds check of their loads and stores. Prints "ok <checks>".
#include <cstdio>
#include <set>
#include <utility>
#include <vector>

#include "../../staticfusion_amd/csrc/sf_region_walk.h"

static int fail_at(const char *what, int rows, int cols, long long at) {
    std::printf("FAIL: %s at %d x %d, %lld\n", what, rows, cols, at);
    return 1;
}

int main() {
    long long checked = 0;
    const int sizes[][2] = {{1, 1},   {1, 9},   {9, 1},    {5, 7},    {37, 53},  {64, 48},   {130, 66}, {240, 320}, {65, 33},  {64, 32},  {63, 31},
                            {128, 64}, {129, 65}, {60, 80}, {4096, 1}, {1, 4096}, {4096, 64}, {64, 4096}, {480, 640}, {257, 255}, {4096, 4096}};
    for (const auto &s : sizes) {
        const int rows = s[0], cols = s[1];
        const RgGeom g = rg_geometry(rows, cols);
        const bool full = (long long)rows * cols <= 400000;  // the exhaustive parts; the largest sizes get the sampled ones
        if (g.px != rows * cols || g.tiles_v != (rows + SFR_TV - 1) / SFR_TV || g.tiles_u != (cols + SFR_TU - 1) / SFR_TU || g.pxs % SFR_RUN || g.pxs < g.px ||
            g.pxs >= g.px + SFR_RUN || g.blocks * SFR_NB < g.px || (g.blocks - 1) * SFR_NB >= g.px || SFR_NB % 4 || g.pxs % 4)
            return fail_at("geometry", rows, cols, 0);
        // ---- tiles: what sfr_tile_kernel's lanes address
        if (full) {
            std::vector<unsigned char> seen((size_t)g.px, 0);
            for (int t = 0; t < g.tiles_v * g.tiles_u; t++) {
                const int v0 = (t % g.tiles_v) * SFR_TV, u0 = (t / g.tiles_v) * SFR_TU;
                for (int tid = 0; tid < SFR_NT; tid++)
                    for (int j = 0; j < SFR_TV * SFR_TU / SFR_NT; j++) {
                        const int lv = tid & (SFR_TV - 1), lu = tid / SFR_TV + (SFR_NT / SFR_TV) * j;
                        const int v = v0 + lv, u = u0 + lu, idx = lu * SFR_TV + lv;
                        if (idx < 0 || idx >= SFR_TV * SFR_TU || lu >= SFR_TU) return fail_at("tile index", rows, cols, idx);
                        // a root r of the tile goes back to the pixel it came from
                        if ((v0 + (idx & (SFR_TV - 1))) != v || (u0 + idx / SFR_TV) != u) return fail_at("tile root", rows, cols, idx);
                        if (v < rows && u < cols) {
                            const long long i = v + (long long)u * rows;
                            if (i >= g.px || seen[(size_t)i]++) return fail_at("tile cover", rows, cols, i);
                        }
                        checked++;
                    }
            }
            for (int i = 0; i < g.px; i++)
                if (seen[(size_t)i] != 1) return fail_at("tile cover", rows, cols, i);
        }
        // ---- border items
        if (g.h_items != (g.tiles_v - 1) * cols || g.items != g.h_items + (g.tiles_u - 1) * rows) return fail_at("item count", rows, cols, g.items);
        std::set<std::pair<int, int>> pairs;  // (smaller index, larger index) the border kernel looks at
        const int stride = full ? 1 : 97;
        for (int item = 0; item < g.items; item += stride) {
            const RgBorder e = rg_border(g, item);
            if (e.v < 0 || e.v >= rows || e.u < 0 || e.u >= cols) return fail_at("item outside", rows, cols, item);
            if (e.horizontal != (item < g.h_items)) return fail_at("item kind", rows, cols, item);
            if (e.horizontal) {
                if (e.v % SFR_TV || e.v == 0 || e.v / SFR_TV - 1 != item / cols || e.u != item % cols) return fail_at("row item", rows, cols, item);
            } else {
                const int j = item - g.h_items;
                if (e.u % SFR_TU || e.u == 0 || e.u / SFR_TU - 1 != j / rows || e.v != j % rows) return fail_at("column item", rows, cols, item);
            }
            if (full) {
                const int cand[6][4] = {{e.v, e.u, e.v - 1, e.u}, {e.v, e.u, e.v - 1, e.u - 1}, {e.v - 1, e.u, e.v, e.u - 1},
                                        {e.v, e.u, e.v, e.u - 1}, {e.v, e.u, e.v - 1, e.u - 1}, {e.v, e.u, e.v + 1, e.u - 1}};
                for (int c = e.horizontal ? 0 : 3; c < (e.horizontal ? 3 : 6); c++) {
                    const int v1 = cand[c][0], u1 = cand[c][1], v2 = cand[c][2], u2 = cand[c][3];
                    if (v1 < 0 || v1 >= rows || u1 < 0 || u1 >= cols) return fail_at("first pixel of a pair outside", rows, cols, item);
                    if (v2 < 0 || v2 >= rows || u2 < 0 || u2 >= cols) continue;  // (rg_border_pair returns)
                    const int i1 = v1 + u1 * rows, i2 = v2 + u2 * rows;
                    pairs.insert({i1 < i2 ? i1 : i2, i1 < i2 ? i2 : i1});
                }
            }
            checked++;
        }
        if (full)  // every 8-neighbour pair across a tile edge is among them
            for (int u = 0; u < cols; u++)
                for (int v = 0; v < rows; v++) {
                    const int nb[4][2] = {{v - 1, u}, {v, u - 1}, {v - 1, u - 1}, {v + 1, u - 1}};
                    for (const auto &q : nb) {
                        if (q[0] < 0 || q[0] >= rows || q[1] < 0) continue;
                        const bool same = q[0] / SFR_TV == v / SFR_TV && q[1] / SFR_TU == u / SFR_TU;
                        const bool have = pairs.count({q[0] + q[1] * rows, v + u * rows}) != 0;
                        if (!same && !have) return fail_at("a pair across a tile edge is missed", rows, cols, v + (long long)u * rows);
                        checked++;
                    }
                }
        // ---- the runs of the flat passes
        const int lanes = (g.px + SFR_RUN - 1) / SFR_RUN;
        for (int lane = 0; lane < lanes; lane += (full ? 1 : 1009)) {
            const int i0 = lane * SFR_RUN;
            if (i0 + SFR_RUN > g.pxs) return fail_at("a run leaves the stride", rows, cols, i0);
            RgRun at;
            at.start(i0, rows);
            for (int j = 0; j < SFR_RUN && i0 + j < g.px; j++) {
                if (at.v != (i0 + j) % rows || at.u != (i0 + j) / rows || at.u >= cols) return fail_at("run", rows, cols, i0 + j);
                at.step(rows);
                checked++;
            }
        }
        // the last lane of all
        {
            const int i0 = (lanes - 1) * SFR_RUN;
            RgRun at;
            at.start(i0, rows);
            if (i0 >= g.px || i0 + SFR_RUN > g.pxs || at.v != i0 % rows || at.u != i0 / rows) return fail_at("last run", rows, cols, i0);
        }
    }
    std::printf("ok %lld\n", checked);
    return 0;
}
