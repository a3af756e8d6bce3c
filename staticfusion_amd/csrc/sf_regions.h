// sf_regions.h — device code of include/sf_regions.h (host side: sf_hip_regions.hip): connected components of the moving
// pixels of many frames per call, numbered in index order, with one integer record per region. Entry = blockIdx.y (the scan:
// blockIdx.x). Seven kernels, one launch each on the handle's stream; what needs a grid-wide order is a launch boundary, and
// NO WORKGROUP EVER WAITS FOR ANOTHER: there is no loop in here that ends on a value another workgroup writes.
//
// Union-find by minimum index. A provisional label P[i] is the index of another pixel of i's component with P[i] <= i; a
// root has P[i] == i. find() walks P, strictly descending, so it takes at most i steps whatever other lanes do meanwhile
// (they only ever lower entries). union(a, b) finds both roots and lowers the larger one onto the smaller with atomicMin;
// when another lane got there first, the returned value is that lane's smaller target and the loop goes on from it: root(a) +
// root(b) falls strictly with every trip. The root of a component is its smallest index whatever the order of the merges,
// which is `first` of the header; numbering by ascending first is an exclusive scan in index order.
//
//   1 sfr_tile_kernel     a tile of 64 rows x 32 columns per workgroup: reads depth (and b) once, lanes down v; masked depth
//                         and labels of the tile in LDS (16 KB); the vertical runs of a column come from one ballot, the
//                         links to the left column that the runs do not already imply are merged with LDS atomics; writes
//                         the tile-resolved labels as GLOBAL pixel indices (-1 outside the mask) and zeroes the counts
//   2 sfr_border_kernel   one lane per pixel of a tile's first row / first column: the links that cross a tile edge, merged in
//                         the global label image with global atomicMin
//   3 sfr_flatten_kernel  every label becomes its root; the size of a component is counted at its root (one atomic per run
//                         of equal roots among a lane's 8 consecutive pixels)
//   4 sfr_count_kernel    per 1024 pixels: how many roots are regions (n >= min_pixels); n_mask and n_components
//   5 sfr_scan_kernel     block_counts_scan: R; the summary; zeroes the records n_written .. max_regions - 1
//   6 sfr_number_kernel   region numbers at the roots (the count image is reused for them), n and first of the records
//   7 sfr_final_kernel    reads depth and b of the masked pixels again: the label image, box, depth range and sums of the
//                         records (integer atomics, one set per wave for the region most of its lanes lie in)
#pragma once
#include "../../include/sf_regions.h"
#include "sf_device_common.h"
#include "sf_region_walk.h"

struct RgArgs {
    const float *depth, *b;  // rows x cols column-major; b null without use_b
    int *labels;             // the label image of the entry, or null
    float z_max, b_max, dz_abs, dz_rel;
    int conn8, min_pixels, use_b, pad;
};

__device__ __forceinline__ bool rg_linked(float zp, float zq, float dz_abs, float dz_rel) { return fabsf(zp - zq) <= dz_abs + dz_rel * fminf(zp, zq); }

// both depths are in the mask (masked depth: 0 outside) and linked
__device__ __forceinline__ bool rg_both_linked(float zp, float zq, const RgArgs &a) { return zp > 0.f && zq > 0.f && rg_linked(zp, zq, a.dz_abs, a.dz_rel); }

// ---- union-find in LDS (one tile) -----------------------------------------------------------------------------------------
__device__ __forceinline__ int rg_find_lds(const volatile int *L, int x) {
    int p;
    while ((p = L[x]) != x) x = p;  // p < x
    return x;
}
__device__ __forceinline__ void rg_union_lds(int *L, int a, int b) {
    for (;;) {
        a = rg_find_lds(L, a);
        b = rg_find_lds(L, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(&L[a], b);
        if (old == a) return;  // a was a root and now hangs below b
        a = old;               // another lane lowered L[a] first: old < a, and its component joins b's
    }
}

__global__ __launch_bounds__(SFR_NT) void sfr_tile_kernel(const RgArgs *args, RgGeom g, int *prov, int *cnt) {
    __shared__ float zt[SFR_TV * SFR_TU];  // masked depth: 0 outside the mask (and outside the image)
    __shared__ int L[SFR_TV * SFR_TU];     // tile index lv + lu * SFR_TV: ordered like the pixel index
    const RgArgs a = args[blockIdx.y];
    const int tid = threadIdx.x, lv = tid & (SFR_TV - 1), cg = tid / SFR_TV;
    const int tv = (int)blockIdx.x % g.tiles_v, tu = (int)blockIdx.x / g.tiles_v;
    const int v0 = tv * SFR_TV, u0 = tu * SFR_TU, v = v0 + lv;
    constexpr int PER = SFR_TV * SFR_TU / SFR_NT, CSTEP = SFR_NT / SFR_TV;
    float z[PER], bf[PER];
#pragma unroll
    for (int j = 0; j < PER; j++) {
        const int u = u0 + cg + CSTEP * j;
        const bool in = v < g.rows && u < g.cols;
        z[j] = in ? a.depth[v + u * g.rows] : 0.f;
        bf[j] = (in && a.use_b) ? a.b[v + u * g.rows] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < PER; j++) {
        const int idx = (cg + CSTEP * j) * SFR_TV + lv;
        const bool m = z[j] > 0.f && z[j] <= a.z_max && (a.use_b ? bf[j] < a.b_max : true);
        zt[idx] = m ? z[j] : 0.f;
        L[idx] = idx;
    }
    __syncthreads();
    // A column of the tile is the 64 lanes of one wave: the vertical runs of linked pixels need no atomics. A lane whose
    // pixel is not linked to the one above begins a run, and every pixel's label is the beginning of its run.
#pragma unroll
    for (int j = 0; j < PER; j++) {
        const int lu = cg + CSTEP * j, idx = lu * SFR_TV + lv;
        const bool up = lv > 0 && rg_both_linked(zt[idx], zt[idx - 1], a);
        const unsigned long long begins = __ballot(!up) & ((2ull << lv) - 1ull);  // at or above this lane; lane 0 always begins one
        L[idx] = lu * SFR_TV + (63 - __clzll((long long)begins));
    }
    __syncthreads();
    // The links to the column on the left. A link whose ends are already joined by two or three links that this pass or the
    // runs above merge is skipped: p - q (left) when p and q are both linked upwards and the two pixels above are linked; a
    // diagonal when one of the two L-shaped paths round it is linked. What a skip relies on lies in the same tile, one row
    // up or in the runs, never on a diagonal, so the reliance ends at the tile's first row, where nothing is skipped.
#pragma unroll
    for (int j = 0; j < PER; j++) {
        const int lu = cg + CSTEP * j, idx = lu * SFR_TV + lv;
        const float zp = zt[idx];
        if (!(zp > 0.f) || lu == 0) continue;
        const float za = lv > 0 ? zt[idx - 1] : 0.f, zq = zt[idx - SFR_TV], zc = lv > 0 ? zt[idx - SFR_TV - 1] : 0.f;
        const bool pa = rg_both_linked(zp, za, a), pq = rg_both_linked(zp, zq, a), qc = rg_both_linked(zq, zc, a), ac = rg_both_linked(za, zc, a);
        if (pq && !(pa && qc && ac)) rg_union_lds(L, idx, idx - SFR_TV);
        if (a.conn8) {
            if (rg_both_linked(zp, zc, a) && !((pa && ac) || (pq && qc))) rg_union_lds(L, idx, idx - SFR_TV - 1);
            const float zd = lv < SFR_TV - 1 ? zt[idx - SFR_TV + 1] : 0.f, ze = lv < SFR_TV - 1 ? zt[idx + 1] : 0.f;
            if (rg_both_linked(zp, zd, a) && !((pq && rg_both_linked(zq, zd, a)) || (rg_both_linked(zp, ze, a) && rg_both_linked(ze, zd, a))))
                rg_union_lds(L, idx, idx - SFR_TV + 1);
        }
    }
    __syncthreads();
    const size_t base = (size_t)blockIdx.y * g.pxs;
#pragma unroll
    for (int j = 0; j < PER; j++) {
        const int lu = cg + CSTEP * j, u = u0 + lu, idx = lu * SFR_TV + lv;
        if (v < g.rows && u < g.cols) {
            int out = -1;
            if (zt[idx] > 0.f) {
                const int r = rg_find_lds(L, idx);
                out = (v0 + (r & (SFR_TV - 1))) + (u0 + r / SFR_TV) * g.rows;
            }
            prov[base + v + u * g.rows] = out;
            cnt[base + v + u * g.rows] = 0;
        }
    }
}

// ---- union-find in the global label image (the tile borders) ----------------------------------------------------------------
__device__ __forceinline__ int rg_find_global(int *P, int x) {
    int p;
    while ((p = __hip_atomic_load(&P[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != x) x = p;  // p < x
    return x;
}
__device__ __forceinline__ void rg_union_global(int *P, int a, int b) {
    for (;;) {
        a = rg_find_global(P, a);
        b = rg_find_global(P, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = __hip_atomic_fetch_min(&P[a], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == a) return;
        a = old;  // old < a: see rg_union_lds
    }
}

// pixel (v1, u1) is inside the image; (v2, u2) may lie outside
__device__ __forceinline__ void rg_border_pair(const RgArgs &a, const RgGeom &g, int *P, int v1, int u1, int v2, int u2) {
    if (v2 < 0 || v2 >= g.rows || u2 < 0 || u2 >= g.cols) return;
    const int i1 = v1 + u1 * g.rows, i2 = v2 + u2 * g.rows;
    if (P[i1] < 0 || P[i2] < 0) return;  // (the sign of a label is the mask and never changes)
    if (rg_linked(a.depth[i1], a.depth[i2], a.dz_abs, a.dz_rel)) rg_union_global(P, i1, i2);
}

__global__ __launch_bounds__(SFR_NT) void sfr_border_kernel(const RgArgs *args, RgGeom g, int *prov) {
    const int item = (int)blockIdx.x * SFR_NT + (int)threadIdx.x;
    if (item >= g.items) return;
    const RgArgs a = args[blockIdx.y];
    int *P = prov + (size_t)blockIdx.y * g.pxs;
    const RgBorder e = rg_border(g, item);
    if (e.horizontal) {  // the links between row v - 1 and row v
        rg_border_pair(a, g, P, e.v, e.u, e.v - 1, e.u);
        if (a.conn8) {
            rg_border_pair(a, g, P, e.v, e.u, e.v - 1, e.u - 1);
            rg_border_pair(a, g, P, e.v - 1, e.u, e.v, e.u - 1);
        }
    } else {  // the links between column u - 1 and column u
        rg_border_pair(a, g, P, e.v, e.u, e.v, e.u - 1);
        if (a.conn8) {
            rg_border_pair(a, g, P, e.v, e.u, e.v - 1, e.u - 1);
            rg_border_pair(a, g, P, e.v, e.u, e.v + 1, e.u - 1);
        }
    }
}

// ---- flatten and count -------------------------------------------------------------------------------------------------------
typedef int __attribute__((ext_vector_type(4))) rg_int4;

// A lane's SFR_RUN labels (the entry's stride is a multiple of SFR_RUN, so the two loads stay inside the block)
__device__ __forceinline__ void rg_load_run(const int *P, int i0, int lab[SFR_RUN]) {
    const rg_int4 lo = *(const rg_int4 *)(P + i0), hi = *(const rg_int4 *)(P + i0 + 4);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        lab[j] = lo[j];
        lab[4 + j] = hi[j];
    }
}

// No lane writes a root's label here, and a label that is rewritten goes from one ancestor to the root: a walk that reads
// the old or the new value ends at the same root.
__global__ __launch_bounds__(SFR_NT) void sfr_flatten_kernel(RgGeom g, int *prov, int *cnt) {
    const int i0 = ((int)blockIdx.x * SFR_NT + (int)threadIdx.x) * SFR_RUN;
    if (i0 >= g.px) return;
    int *P = prov + (size_t)blockIdx.y * g.pxs, *C = cnt + (size_t)blockIdx.y * g.pxs;
    int lab[SFR_RUN];
    rg_load_run(P, i0, lab);
    int cur = -1, n = 0;
#pragma unroll
    for (int j = 0; j < SFR_RUN; j++) {
        const int p = lab[j];
        if (i0 + j >= g.px || p < 0) continue;
        int r = p, q;
        while ((q = P[r]) != r) r = q;  // q < r
        if (r != p) P[i0 + j] = r;
        if (r == cur) {
            n++;
        } else {
            if (n) atomicAdd(&C[cur], n);
            cur = r;
            n = 1;
        }
    }
    if (n) atomicAdd(&C[cur], n);
}

// ---- numbering ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SFR_NT) void sfr_count_kernel(const RgArgs *args, RgGeom g, const int *prov, const int *cnt, int *block_counts,
                                                           sfr_summary *summaries) {
    __shared__ int part[3][SFR_NT / 64];
    const int tid = threadIdx.x, i0 = (int)blockIdx.x * SFR_NB + tid * 4;
    const int min_pixels = args[blockIdx.y].min_pixels;
    const int *P = prov + (size_t)blockIdx.y * g.pxs, *C = cnt + (size_t)blockIdx.y * g.pxs;
    int n_mask = 0, n_comp = 0, n_reg = 0;
    if (i0 < g.px) {
        const rg_int4 lab = *(const rg_int4 *)(P + i0), c = *(const rg_int4 *)(C + i0);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (i0 + j >= g.px) continue;
            n_mask += lab[j] >= 0;
            if (lab[j] == i0 + j) {
                n_comp++;
                n_reg += c[j] >= min_pixels;
            }
        }
    }
    n_mask = wave_sum(n_mask);
    n_comp = wave_sum(n_comp);
    n_reg = wave_sum(n_reg);
    if ((tid & 63) == 0) {
        part[0][tid >> 6] = n_mask;
        part[1][tid >> 6] = n_comp;
        part[2][tid >> 6] = n_reg;
    }
    __syncthreads();
    if (tid == 0) {
        int s[3] = {0, 0, 0};
        for (int w = 0; w < SFR_NT / 64; w++)
            for (int k = 0; k < 3; k++) s[k] += part[k][w];
        block_counts[(size_t)blockIdx.y * g.blocks + blockIdx.x] = s[2];
        if (s[0]) atomicAdd(&summaries[blockIdx.y].n_mask, s[0]);
        if (s[1]) atomicAdd(&summaries[blockIdx.y].n_components, s[1]);
    }
}

// one workgroup per entry: the block counts become offsets, the total is R
__global__ __launch_bounds__(SFR_SCAN_NT) void sfr_scan_kernel(RgGeom g, int *block_counts, int max_regions, sfr_summary *summaries, sfr_region *regions) {
    const int q = blockIdx.x, tid = threadIdx.x;
    const int total = block_counts_scan(block_counts + (size_t)q * g.blocks, g.blocks);
    const int written = total < max_regions ? total : max_regions;
    if (tid == 0) {
        summaries[q].n_regions = total;
        summaries[q].n_written = written;
    }
    constexpr int WORDS = (int)(sizeof(sfr_region) / sizeof(long long));
    long long *r = (long long *)(regions + (size_t)q * max_regions);
    for (int k = written * WORDS + tid; k < max_regions * WORDS; k += SFR_SCAN_NT) r[k] = 0;
}

__global__ __launch_bounds__(SFR_NT) void sfr_number_kernel(const RgArgs *args, RgGeom g, const int *prov, int *cnt, const int *block_counts, int max_regions,
                                                            sfr_region *regions) {
    __shared__ int wsum[SFR_NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i0 = (int)blockIdx.x * SFR_NB + tid * 4;
    const int min_pixels = args[blockIdx.y].min_pixels;
    const int *P = prov + (size_t)blockIdx.y * g.pxs;
    int *C = cnt + (size_t)blockIdx.y * g.pxs;
    bool root[4] = {false, false, false, false};
    int size[4] = {0, 0, 0, 0};
    int mine = 0;
    if (i0 < g.px) {
        const rg_int4 lab = *(const rg_int4 *)(P + i0), c = *(const rg_int4 *)(C + i0);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            root[j] = i0 + j < g.px && lab[j] == i0 + j;
            size[j] = c[j];
            mine += root[j] && c[j] >= min_pixels;
        }
    }
    int incl = mine;
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(incl, off, 64);
        if (lane >= off) incl += o;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int k = block_counts[(size_t)blockIdx.y * g.blocks + blockIdx.x] + incl - mine;  // regions before this lane's pixels
    for (int w = 0; w < wave; w++) k += wsum[w];
    sfr_region *rec = regions + (size_t)blockIdx.y * max_regions;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (!root[j]) continue;
        if (size[j] < min_pixels) {
            C[i0 + j] = 0;  // a small component: its pixels get -1
            continue;
        }
        C[i0 + j] = ++k;
        if (k <= max_regions) {
            sfr_region r;
            r.n = size[j];
            r.first = i0 + j;
            r.v_min = r.u_min = r.z_min = 0x7fffffff;
            r.v_max = r.u_max = r.z_max = -1;
            r.sum_v = r.sum_u = r.sum_z = r.sum_b = 0;
            rec[k - 1] = r;
        }
    }
}

// ---- labels and statistics -----------------------------------------------------------------------------------------------
struct RgAcc {
    int k, v_min, v_max, u_min, u_max, z_min, z_max;
    long long sum_v, sum_u, sum_z, sum_b;
    __device__ __forceinline__ void reset(int region) {
        k = region;
        v_min = u_min = z_min = 0x7fffffff;
        v_max = u_max = z_max = -1;
        sum_v = sum_u = sum_z = sum_b = 0;
    }
    __device__ __forceinline__ void flush(sfr_region *rec, int max_regions) const {
        if (k < 1 || k > max_regions || v_max < 0) return;
        sfr_region *r = rec + (k - 1);
        atomicMin(&r->v_min, v_min);
        atomicMax(&r->v_max, v_max);
        atomicMin(&r->u_min, u_min);
        atomicMax(&r->u_max, u_max);
        atomicMin(&r->z_min, z_min);
        atomicMax(&r->z_max, z_max);
        atomicAdd((unsigned long long *)&r->sum_v, (unsigned long long)sum_v);
        atomicAdd((unsigned long long *)&r->sum_u, (unsigned long long)sum_u);
        atomicAdd((unsigned long long *)&r->sum_z, (unsigned long long)sum_z);
        if (sum_b) atomicAdd((unsigned long long *)&r->sum_b, (unsigned long long)sum_b);
    }
};

__device__ __forceinline__ int rg_wave_min(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = min(v, __shfl_xor(v, d, 64));
    return v;
}
__device__ __forceinline__ int rg_wave_max(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
    return v;
}
// Every lane stays to the end (lanes past the image hold nothing): the wave adds what its lanes hold for one region -- the
// region of its first lane that holds any -- with shuffles and one lane writes it; lanes that end in another region write
// their own. The sums are integers, so who adds what changes nothing.
__global__ __launch_bounds__(SFR_NT) void sfr_final_kernel(const RgArgs *args, RgGeom g, const int *prov, const int *cnt, int max_regions, sfr_region *regions) {
    const int i0 = ((int)blockIdx.x * SFR_NT + (int)threadIdx.x) * SFR_RUN;
    const RgArgs a = args[blockIdx.y];
    const int *P = prov + (size_t)blockIdx.y * g.pxs, *C = cnt + (size_t)blockIdx.y * g.pxs;
    sfr_region *rec = regions + (size_t)blockIdx.y * max_regions;
    RgAcc acc;
    acc.reset(0);
    if (i0 < g.px) {
        int lab[SFR_RUN];
        rg_load_run(P, i0, lab);
        float z[SFR_RUN], bf[SFR_RUN];
#pragma unroll
        for (int j = 0; j < SFR_RUN; j++) {
            const bool in = i0 + j < g.px && lab[j] >= 0 && max_regions > 0;
            z[j] = in ? a.depth[i0 + j] : 0.f;
            bf[j] = (in && a.use_b) ? a.b[i0 + j] : 0.f;
        }
        RgRun at;
        at.start(i0, g.rows);
        int cur = -1;
#pragma unroll
        for (int j = 0; j < SFR_RUN; j++) {
            if (i0 + j >= g.px) break;
            const int p = lab[j];
            int out = 0;
            if (p >= 0) {
                if (p != cur) {
                    acc.flush(rec, max_regions);
                    cur = p;
                    acc.reset(C[p]);
                }
                out = acc.k ? acc.k : -1;
                if (acc.k >= 1 && acc.k <= max_regions) {
                    const int zq = (int)rintf(z[j] * 1024.f);
                    acc.v_min = min(acc.v_min, at.v);
                    acc.v_max = max(acc.v_max, at.v);
                    acc.u_min = min(acc.u_min, at.u);
                    acc.u_max = max(acc.u_max, at.u);
                    acc.z_min = min(acc.z_min, zq);
                    acc.z_max = max(acc.z_max, zq);
                    acc.sum_v += at.v;
                    acc.sum_u += at.u;
                    acc.sum_z += zq;
                    if (a.use_b) acc.sum_b += (int)rintf(fminf(fmaxf(bf[j], 0.f), 1.f) * 4096.f);
                }
            }
            if (a.labels) a.labels[i0 + j] = out;
            at.step(g.rows);
        }
    }
    const bool holds = acc.k >= 1 && acc.k <= max_regions && acc.v_max >= 0;
    const unsigned long long holders = __ballot(holds);
    if (holders == 0) return;  // (the whole wave)
    const int leader = __ffsll((long long)holders) - 1;
    const int k0 = __shfl(acc.k, leader, 64);
    const bool join = holds && acc.k == k0;
    if (holds && !join) acc.flush(rec, max_regions);
    RgAcc w;
    w.k = k0;
    w.v_min = rg_wave_min(join ? acc.v_min : 0x7fffffff);
    w.v_max = rg_wave_max(join ? acc.v_max : -1);
    w.u_min = rg_wave_min(join ? acc.u_min : 0x7fffffff);
    w.u_max = rg_wave_max(join ? acc.u_max : -1);
    w.z_min = rg_wave_min(join ? acc.z_min : 0x7fffffff);
    w.z_max = rg_wave_max(join ? acc.z_max : -1);
    w.sum_v = wave_sum(join ? acc.sum_v : 0);
    w.sum_u = wave_sum(join ? acc.sum_u : 0);
    w.sum_z = wave_sum(join ? acc.sum_z : 0);
    w.sum_b = wave_sum(join ? acc.sum_b : 0);
    if (((int)threadIdx.x & 63) == leader) w.flush(rec, max_regions);
}
