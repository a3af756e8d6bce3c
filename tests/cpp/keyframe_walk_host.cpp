// The item walk of sfk_encode_kernel (staticfusion_amd/csrc/sf_keyframe_walk.h) held to the divisions it replaces, on the host:
// for every geometry below, every load width it admits and every lane, the walk visits exactly the items tid, tid + 256, ...
// below the item count, each at the column, row and cell the divisions give, and ends there. Every address the kernel forms
// comes from these counters, so this is the bounds check of its loads. Prints "ok <items>".
#include <cstdio>
#include <initializer_list>

#include "../../staticfusion_amd/csrc/sf_keyframe_walk.h"

int main() {
    long long checked = 0;
    const int sizes[][3] = {{8, 8, 8}, {1, 1, 1}, {5, 7, 3}, {53, 37, 8}, {64, 48, 4}, {130, 66, 64}, {240, 320, 8}, {240, 320, 5}, {60, 80, 4}, {60, 80, 6},
                            {4096, 64, 64}, {64, 4096, 64}, {4096, 1, 1}, {1, 4096, 1}, {4095, 3, 3}, {480, 640, 10}, {6, 1000, 2}, {2, 4096, 2}, {128, 128, 2},
                            {4096, 4096, 64}, {257, 255, 16}, {256, 256, 4}};
    for (const auto &s : sizes) {
        const int rows = s[0], cols = s[1], cell = s[2];
        const int gr = rows / cell, gc = cols / cell;
        if (gr * gc < 1 || gr * gc > 4096) {
            std::printf("FAIL: %d x %d at cell %d is no legal grid\n", rows, cols, cell);
            return 1;
        }
        for (int w : {1, 2, 4}) {
            if (cell % w || rows % w) continue;
            const KfGeom g = kf_geometry(rows, cell, gr, gc, w);
            const int ipc = gr * cell / w;
            const long long items = (long long)ipc * gc * cell;
            for (int tid = 0; tid < SFK_NT; tid++) {
                KfWalk at;
                at.start(g, tid);
                long long item = tid;
                while (at.inside(g)) {
                    const int u = (int)(item / ipc), v = (int)(item % ipc) * w;
                    const int gu = at.uc * cell + at.ur, gv = (at.kc * g.cpw + at.kr) * w;
                    if (item >= items || gu != u || gv != v || at.kc != v / cell || at.uc != u / cell || at.kr >= g.cpw || at.ur >= cell || at.kc >= gr ||
                        gu >= gc * cell || gv + w > gr * cell) {
                        std::printf("FAIL: %d x %d cell %d width %d lane %d item %lld of %lld\n", rows, cols, cell, w, tid, item, items);
                        return 1;
                    }
                    checked++;
                    at.step(g);
                    item += SFK_NT;
                }
                if (item < items) {
                    std::printf("FAIL: %d x %d cell %d width %d lane %d ends at item %lld of %lld\n", rows, cols, cell, w, tid, item, items);
                    return 1;
                }
            }
        }
    }
    std::printf("ok %lld\n", checked);
    return 0;
}
