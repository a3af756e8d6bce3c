// sf_region_walk.h — the index arithmetic of the region kernels (sf_regions.h): the tiles of the labelling pass, the items
// of the border pass and the (v, u) counters of a lane that walks consecutive pixel indices. No HIP in here, so that
// tests/cpp/region_walk_host.cpp can hold it to the plain divisions it replaces with a plain C++ compiler: every address the
// kernels form comes from these values.
#pragma once
#ifdef __HIPCC__
#define RG_HD __host__ __device__
#else
#define RG_HD
#endif

#define SFR_NT 256    // threads of every region kernel but the scan
#define SFR_TV 64     // rows of a tile: down v, which is along memory (one wave reads 256 contiguous bytes of a column)
#define SFR_TU 32     // columns of a tile
#define SFR_RUN 8     // consecutive pixel indices a lane of the flat passes handles
#define SFR_NB 1024   // pixels per workgroup of the numbering passes: SFR_NT lanes x 4
#define SFR_SCAN_NT 1024  // threads of the scan (block_counts_scan works on chunks of 1024)

// Geometry of a call, filled on the host: the image, its tiles and the items of the border pass.
struct RgGeom {
    int rows, cols, px;
    int tiles_v, tiles_u;  // ceil(rows / SFR_TV), ceil(cols / SFR_TU); tile t is (t % tiles_v, t / tiles_v)
    int h_items;           // (tiles_v - 1) * cols: the pixels of the first row of every tile row but the first
    int items;             // h_items + (tiles_u - 1) * rows: and of the first column of every tile column but the first
    int pxs;               // px rounded up to a multiple of SFR_RUN: the stride of an entry in the scratch images
    int blocks;            // ceil(px / SFR_NB)
};

static inline RgGeom rg_geometry(int rows, int cols) {
    RgGeom g;
    g.rows = rows;
    g.cols = cols;
    g.px = rows * cols;
    g.tiles_v = (rows + SFR_TV - 1) / SFR_TV;
    g.tiles_u = (cols + SFR_TU - 1) / SFR_TU;
    g.h_items = (g.tiles_v - 1) * cols;
    g.items = g.h_items + (g.tiles_u - 1) * rows;
    g.pxs = (g.px + SFR_RUN - 1) / SFR_RUN * SFR_RUN;
    g.blocks = (g.px + SFR_NB - 1) / SFR_NB;
    return g;
}

// The pixel of a border item and the edge it lies on: horizontal items are (v, u) with v a multiple of SFR_TV, v > 0, whose
// neighbours in row v - 1 lie in another tile; vertical items have u a multiple of SFR_TU, u > 0, and look at column u - 1.
struct RgBorder {
    int v, u;
    bool horizontal;
};
RG_HD static inline RgBorder rg_border(const RgGeom &g, int item) {
    RgBorder b;
    if (item < g.h_items) {
        const int k = item / g.cols;
        b.v = (k + 1) * SFR_TV;
        b.u = item - k * g.cols;
        b.horizontal = true;
    } else {
        const int j = item - g.h_items;
        const int k = j / g.rows;
        b.u = (k + 1) * SFR_TU;
        b.v = j - k * g.rows;
        b.horizontal = false;
    }
    return b;
}

// (v, u) of pixel index i = v + u * rows, stepped to i + 1 without a division
struct RgRun {
    int v, u;
    RG_HD void start(int i, int rows) {
        u = i / rows;
        v = i - u * rows;
    }
    RG_HD void step(int rows) {
        if (++v == rows) {
            v = 0;
            u++;
        }
    }
};
