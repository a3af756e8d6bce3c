// sf_score.h — device code of include/sf_score.h (host side: sf_hip_score.hip): the frame-to-map agreement counts of a batch
// of (map, view, frame) entries. The map of an entry has been drawn into its key image by the drawing stage of the views
// (sfv_draw_keys: rays, clear, splat, large sprites); sfs_score_kernel is the one launch after it. Table entry blockIdx.y,
// the grid sized for the largest view, workgroups beyond their entry's extent leave at once.
//
// The kernel is flat over the column-major pixel index: the key image, the ray table and the frame images (column-major like
// every image of sf.h) are all read along lanes. The winner of a pixel is evaluated again from its key, as
// sfv_resolve_kernel does, so zm is the same float the depth image of a render holds. The seven predicates are counted with
// wave ballots (scalar popcounts), the three sums are kept per lane in 64-bit integers, reduced across the wave with
// shuffles, across the four waves through 320 bytes of LDS, and added to the entry's record with 64-bit integer atomics:
// at most once per field per workgroup, and not at all for a field whose workgroup total is 0. Integer sums: the record does
// not depend on the order of arrival. No image is written unless the class image is asked for.
#pragma once
#include "sf_view_common.h"

struct ScoreArgs {
    const float *depth, *grey, *b;  // rows x cols column-major; grey / b are read only with their flag
    float tol_abs, tol_rel, max_residual, b_min;
    int use_grey, use_b;
    long long *score;               // the entry's sfs_score: 12 x int64, zeroed before the launch
    uint8_t *cls;                   // rows x cols column-major, or null
};

#define SFS_NT 256
#define SFS_PER_THREAD 4  // pixels per lane: a workgroup covers 1024 consecutive pixels, a QVGA view sends 75 x 10 atomics
#define SFS_FIELDS 10

__global__ __launch_bounds__(SFS_NT) void sfs_score_kernel(const ViewArgs *vtab, const ScoreArgs *stab) {
    __shared__ long long part[SFS_NT / 64][SFS_FIELDS];
    const ViewArgs &a = vtab[blockIdx.y];
    const ScoreArgs &p = stab[blockIdx.y];
    const int px = a.rows * a.cols;  // <= 2^24
    const int base = (int)blockIdx.x * (SFS_NT * SFS_PER_THREAD);
    if (base >= px) return;  // a workgroup of a larger view of the batch
    const int tid = threadIdx.x;
    long long cnt[7] = {0, 0, 0, 0, 0, 0, 0};  // wave-uniform
    long long s_abs = 0, s_sq = 0, s_grey = 0;
#pragma unroll
    for (int k = 0; k < SFS_PER_THREAD; k++) {
        const int idx = base + k * SFS_NT + tid;  // y + x * rows
        const bool in = idx < px;
        bool fv = false, w = true, drawn = false;
        float zf = 0.f, zm = 0.f;
        unsigned c = 0u;
        if (in) {
            zf = as_global(p.depth)[idx];
            fv = zf > 0.f;
            if (p.use_b) w = as_global(p.b)[idx] > p.b_min;
            const unsigned long long key = as_global(a.keys)[idx];
            if (key != SFV_EMPTY) {
                drawn = true;
                const int s = (int)(unsigned)(key & 0xffffffffull);
                const int x = idx / a.rows, y = idx - x * a.rows;
                PV3 h, n;
                float rad, depth;
                sfv_to_camera(a, s, h, n, rad);
                surfel_fragment(a, h, n, rad, x, y, zm, depth);
                c = (unsigned)(int)as_global(a.surfels)[(size_t)s * 12 + 4] & 0xffffffu;  // color.glsl decodeColor
            }
        }
        const bool F = fv && w, masked = fv && !w, both = F && drawn;
        const float r = zf - zm;
        const float tol = p.tol_abs + p.tol_rel * zm;
        const bool inlier = both && fabsf(r) <= tol, front = both && r < -tol, behind = both && r > tol;
        if (both) {
            const long long q = (long long)rintf(fminf(fabsf(r), p.max_residual) * 16384.f);
            s_abs += q;
            s_sq += q * q;
        }
        if (inlier && p.use_grey) {
            const float norm = 1.f / 255.f;
            const float fr = float((c >> 16) & 0xffu) * norm, fg = float((c >> 8) & 0xffu) * norm, fb = float(c & 0xffu) * norm;
            const float gm = (0.299f * fr + 0.587f * fg) + 0.114f * fb;
            const float gf = as_global(p.grey)[idx];
            s_grey += (long long)rintf(fminf(fabsf(gf - gm), 1.f) * 65536.f);
        }
        cnt[0] += __popcll(__ballot(F));
        cnt[1] += __popcll(__ballot(masked));
        cnt[2] += __popcll(__ballot(drawn));
        cnt[3] += __popcll(__ballot(both));
        cnt[4] += __popcll(__ballot(inlier));
        cnt[5] += __popcll(__ballot(front));
        cnt[6] += __popcll(__ballot(behind));
        if (in && p.cls) {
            uint8_t code = drawn ? 2 : 0;
            if (masked) code = 6;
            else if (inlier) code = 3;
            else if (front) code = 4;
            else if (behind) code = 5;
            else if (F) code = drawn ? 2 : 1;
            p.cls[idx] = code;
        }
    }
    s_abs = wave_sum(s_abs);
    s_sq = wave_sum(s_sq);
    s_grey = wave_sum(s_grey);
    const int wave = tid >> 6, lane = tid & 63;
    if (lane == 0) {
#pragma unroll
        for (int f = 0; f < 7; f++) part[wave][f] = cnt[f];
        part[wave][7] = s_abs;
        part[wave][8] = s_sq;
        part[wave][9] = s_grey;
    }
    __syncthreads();
    if (tid < SFS_FIELDS) {
        long long v = 0;
#pragma unroll
        for (int q = 0; q < SFS_NT / 64; q++) v += part[q][tid];
        if (v) __hip_atomic_fetch_add(as_global(p.score) + tid, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
