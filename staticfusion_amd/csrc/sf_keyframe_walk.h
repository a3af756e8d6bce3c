// sf_keyframe_walk.h — how a lane of sfk_encode_kernel (sf_keyframes.h) walks the pixels of a frame: the geometry the host
// fills and the four counters a lane steps. No HIP in here, so that tests/cpp/keyframe_walk_host.cpp can hold the walk to the
// divisions it replaces with a plain C++ compiler: every address the kernel forms comes from these counters.
#pragma once
#ifdef __HIPCC__
#define KF_HD __host__ __device__
#else
#define KF_HD
#endif

#define SFK_NT 256

// Geometry of an encode launch, filled on the host (kf_geometry): what the walk of the items needs, divisions done once.
struct KfGeom {
    int rows, cell, gr, gc;
    int cpw;       // items per cell and column: cell / W
    int d_kc, d_kr, d_uc, d_ur;  // SFK_NT items further: (d_kc * cpw + d_kr) items down the column and (d_uc * cell + d_ur) columns on
};

// The item a lane is at: column u = uc * cell + ur, rows (kc * cpw + kr) * W .. + W - 1, which lie in cell kc + uc * gr.
struct KfWalk {
    int uc, ur, kc, kr;
    KF_HD void start(const KfGeom &g, int item) {
        const int ipc = g.gr * g.cpw;  // items per column
        const int u = item / ipc, k = item - u * ipc;
        uc = u / g.cell;
        ur = u - uc * g.cell;
        kc = k / g.cpw;
        kr = k - kc * g.cpw;
    }
    KF_HD void step(const KfGeom &g) {  // SFK_NT items further; every sum below stays under twice its modulus
        kr += g.d_kr;
        kc += g.d_kc;
        if (kr >= g.cpw) {
            kr -= g.cpw;
            kc++;
        }
        ur += g.d_ur;
        uc += g.d_uc;
        if (kc >= g.gr) {
            kc -= g.gr;
            ur++;
        }
        if (ur >= g.cell) {
            ur -= g.cell;
            uc++;
        }
    }
    KF_HD bool inside(const KfGeom &g) const { return uc < g.gc; }
};

static inline KfGeom kf_geometry(int rows, int cell, int gr, int gc, int w) {
    KfGeom g{rows, cell, gr, gc, cell / w, 0, 0, 0, 0};
    const int ipc = gr * g.cpw;
    const int du = SFK_NT / ipc, dk = SFK_NT % ipc;
    g.d_kc = dk / g.cpw;
    g.d_kr = dk % g.cpw;
    g.d_uc = du / cell;
    g.d_ur = du % cell;
    return g;
}

