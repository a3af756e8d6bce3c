// sf_view.h — device code of include/sf_view.h (host side: sf_hip_view.hip): a surfel buffer drawn from any pose, with any
// pinhole intrinsics, at any size, into a depth, a colour and an index image. The geometry is ONE target of
// IndexMap::combinedPredict (splat.vert, combo_splat.frag), the very functions the prediction draws with (sf_surfel_geom.h):
// visibility is one 64-bit atomicMin per fragment on (bits of gl_FragDepth) << 32 | surfel index, so the images do not
// depend on the execution order. The argument table and the cull of a view are in sf_view_common.h, which the score kernel
// (sf_score.h) shares; the kernels below are defined once, in the translation unit of sf_hip_view.hip.
//
// Four launches serve a whole batch of views (table entry blockIdx.y, like PredictArgs / WindowArgs): clear, splat (a lane
// per surfel), large sprites (a wave per listed surfel), resolve (a lane per pixel). A fifth, in front, builds the view-ray
// table of every distinct (rows, cols, cx, cy, fx, fy) of the call.
#pragma once
#include "sf_view_common.h"

#define SFV_SPLAT_NT 512
// One target, so the 48 KB that hold the prediction's two tiles of 3072 pixels could hold one of 6144 here -- or the same
// 3072 pixels in 24 KB at a higher occupancy. The kernel needs 45 VGPRs (8 waves per SIMD by registers): with 24 KB four
// 512-thread workgroups are resident per CU (8 waves per SIMD), with 48 KB three (6, the prediction's occupancy). Both were
// built and run alternately (tools/view_bench.py): the small tile is faster in every case, 9 % for
// 256 QVGA views, 3.5 % for a 1280 x 960 orbit where more workgroups leave the LDS path.
#ifndef SFV_SPLAT_TILE  // (an A/B build sets another: tools/build_variant.sh, tools/view_bench.py under SF_HIP_LIB)
#define SFV_SPLAT_TILE 3072
#endif
// A surfel whose clipped sprite has more pixels than this is not walked by its lane: a whole wave draws it (sfv_large_kernel)
#define SFV_LARGE_PIXELS 1024  // 32 x 32
#define SFV_LARGE_NT 256
#define SFV_LARGE_BLOCKS 64    // workgroups per view that walk its list (4 waves each)

__global__ __launch_bounds__(256) void sfv_rays_kernel(const ViewRayArgs *tab) {
    const ViewRayArgs &a = tab[blockIdx.y];
    const int idx = blockIdx.x * 256 + threadIdx.x;  // j + i * rows
    if (idx >= a.rows * a.cols) return;
    const int i = idx / a.rows, j = idx - i * a.rows;
    const PV3 l = surfel_view_ray(i, j, a.cx, a.cy, a.fx, a.fy);
    a.rays[idx] = vfloat4{l.x, l.y, l.z, 0.f};
}

__global__ __launch_bounds__(256) void sfv_clear_kernel(const ViewArgs *tab) {
    const ViewArgs &a = tab[blockIdx.y];
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o < a.rows * a.cols) a.keys[o] = SFV_EMPTY;
    if (o == 0) *a.large_count = 0;
}

// One lane per surfel, the plan of sf_predict_splat_kernel for one target: the workgroup resolves its fragments in an LDS
// tile when the bounding box of its sprites fits and sends the tile's winners to the key image; otherwise one global
// atomicMin per fragment. A sprite of more than SFV_LARGE_PIXELS pixels takes no part in either: it is listed.
__global__ __launch_bounds__(SFV_SPLAT_NT) void sfv_splat_kernel(const ViewArgs *tab) {
    __shared__ unsigned long long tile[SFV_SPLAT_TILE];
    __shared__ int bb[4];
    const ViewArgs &a = tab[blockIdx.y];
    if ((int)blockIdx.x * SFV_SPLAT_NT >= a.count) return;  // a workgroup of a larger map of the batch
    const int tid = threadIdx.x;
    const int s = blockIdx.x * SFV_SPLAT_NT + tid;
    PV3 h{0.f, 0.f, 1.f}, n{0.f, 0.f, 1.f};
    float rad = 0.f;
    int i0 = 0, i1 = -1, j0 = 0, j1 = -1;
    bool valid = s < a.count && sfv_sprite(a, s, h, n, rad, i0, i1, j0, j1);
    if (valid && (i1 - i0 + 1) * (j1 - j0 + 1) > SFV_LARGE_PIXELS) {
        const int slot = __hip_atomic_fetch_add(as_global(a.large_count), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (slot < a.count) a.large_list[slot] = s;  // (always: a surfel is listed once)
        valid = false;
    }
    workgroup_sprite_box(bb, valid, i0, i1, j0, j1);
    const int bi0 = bb[0], bj0 = bb[1], bw = bb[2] - bi0 + 1, bh = bb[3] - bj0 + 1;
    if (bw <= 0 || bh <= 0) return;  // nothing to draw (uniform: read from LDS after the barrier)
    const bool tiled = (long long)bw * bh <= SFV_SPLAT_TILE;
    const bool wide = bw > bh;  // tile layout along the longer side of the box (sf_predict.h)
    if (tiled) {
        for (int q = tid; q < bw * bh; q += SFV_SPLAT_NT) tile[q] = SFV_EMPTY;
        __syncthreads();
    }
    if (valid)
        for (int i = i0; i <= i1; i++)
            for (int j = j0; j <= j1; j++) {
                float z, depth;
                if (!surfel_fragment(a, h, n, rad, i, j, z, depth)) continue;
                const unsigned long long key = surfel_key(depth, s);
                if (tiled) {
                    const int t = wide ? (j - bj0) * bw + (i - bi0) : (i - bi0) * bh + (j - bj0);
                    atomicMin(&tile[t], key);
                } else {
                    __hip_atomic_fetch_min(as_global(a.keys) + (j + (size_t)i * a.rows), key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
    if (!tiled) return;
    __syncthreads();
    for (int q = tid; q < bw * bh; q += SFV_SPLAT_NT) {
        const int i = bi0 + (wide ? q % bw : q / bh), j = bj0 + (wide ? q / bw : q % bh);
        const unsigned long long k = tile[q];
        if (k != SFV_EMPTY) __hip_atomic_fetch_min(as_global(a.keys) + (j + (size_t)i * a.rows), k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// The listed sprites, one wave each: the 64 lanes walk the sprite's pixels in the key image's own (column-major) order, so a
// wave's atomics fall on neighbouring words. A view from 0.4 m at four times QVGA has sprites of 10^5 pixels; one lane
// walking one would hold up its whole workgroup. min is commutative and associative: whichever kernel draws a fragment, the
// key image is the same.
__global__ __launch_bounds__(SFV_LARGE_NT) void sfv_large_kernel(const ViewArgs *tab) {
    const ViewArgs &a = tab[blockIdx.y];
    const int n_listed = min(*a.large_count, a.count);
    const int lane = threadIdx.x & 63;
    const int waves = (int)gridDim.x * (SFV_LARGE_NT / 64);
    for (int e = (int)blockIdx.x * (SFV_LARGE_NT / 64) + (int)(threadIdx.x >> 6); e < n_listed; e += waves) {
        const int s = __builtin_amdgcn_readfirstlane(a.large_list[e]);
        if (s < 0 || s >= a.count) continue;
        PV3 h, n;
        float rad;
        int i0, i1, j0, j1;
        if (!sfv_sprite(a, s, h, n, rad, i0, i1, j0, j1)) continue;  // (it was drawn when it was listed)
        const int hgt = j1 - j0 + 1, total = (i1 - i0 + 1) * hgt;
        const int di = 64 / hgt, dj = 64 - di * hgt;  // a step of 64 pixels in (column, row)
        int i = i0 + lane / hgt, j = j0 + lane % hgt;
        for (int q = lane; q < total; q += 64) {
            float z, depth;
            if (surfel_fragment(a, h, n, rad, i, j, z, depth)) {
                const unsigned long long key = surfel_key(depth, s);
                __hip_atomic_fetch_min(as_global(a.keys) + (j + (size_t)i * a.rows), key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            i += di;
            j += dj;
            if (j > j1) {
                j -= hgt;
                i++;
            }
        }
    }
}

// One lane per pixel: the winning fragment is evaluated again and depth / colour / index are written. A workgroup owns a
// 32 x 32 tile. Phase 1 runs lanes along y, the direction of the column-major key image and ray table; the three results
// cross an LDS tile and phase 2 stores them with lanes along x, the direction of the row-major outputs.
#define SFV_T 32
__global__ __launch_bounds__(256) void sfv_resolve_kernel(const ViewArgs *tab) {
    __shared__ float t_z[SFV_T][SFV_T + 1];
    __shared__ unsigned t_c[SFV_T][SFV_T + 1];
    __shared__ int t_s[SFV_T][SFV_T + 1];
    const ViewArgs &a = tab[blockIdx.y];
    const int tiles_x = (a.cols + SFV_T - 1) / SFV_T, tiles_y = (a.rows + SFV_T - 1) / SFV_T;
    if ((int)blockIdx.x >= tiles_x * tiles_y) return;  // a workgroup of a larger view of the batch
    const int ty = (int)blockIdx.x % tiles_y, tx = (int)blockIdx.x / tiles_y;
    const int x0 = tx * SFV_T, y0 = ty * SFV_T;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int yl = threadIdx.x & 31, xl = (threadIdx.x >> 5) + 8 * k;
        const int x = x0 + xl, y = y0 + yl;
        if (x >= a.cols || y >= a.rows) continue;
        const unsigned long long key = as_global(a.keys)[y + (size_t)x * a.rows];
        float z = 0.f;
        unsigned c = 0u;
        int s = -1;
        if (key != SFV_EMPTY) {
            s = (int)(unsigned)(key & 0xffffffffull);
            PV3 h, n;
            float rad, depth;
            sfv_to_camera(a, s, h, n, rad);
            surfel_fragment(a, h, n, rad, x, y, z, depth);
            if (a.shade == 1) {  // SFV_SHADE_NORMAL
                const float v[3] = {n.x, n.y, n.z};
#pragma unroll
                for (int q = 0; q < 3; q++) {
                    const unsigned b = (unsigned)(uint8_t)(int)rintf(fminf(fmaxf(0.5f * v[q] + 0.5f, 0.f), 1.f) * 255.f);
                    c |= b << (16 - 8 * q);
                }
            } else {
                c = (unsigned)(int)as_global(a.surfels)[(size_t)s * 12 + 4] & 0xffffffu;  // color.glsl decodeColor
            }
        }
        t_z[yl][xl] = z;
        t_c[yl][xl] = c;
        t_s[yl][xl] = s;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int xl = threadIdx.x & 31, yl = (threadIdx.x >> 5) + 8 * k;
        const int x = x0 + xl, y = y0 + yl;
        if (x >= a.cols || y >= a.rows) continue;
        const size_t o = (size_t)y * a.cols + x;
        if (a.depth) a.depth[o] = t_z[yl][xl];
        if (a.index) a.index[o] = t_s[yl][xl];
        if (a.rgb) {
            const unsigned c = t_c[yl][xl];
            a.rgb[o * 3] = (uint8_t)(c >> 16);
            a.rgb[o * 3 + 1] = (uint8_t)(c >> 8);
            a.rgb[o * 3 + 2] = (uint8_t)c;
        }
    }
}
