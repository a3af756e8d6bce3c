// sf_tracks.h — device code of include/sf_tracks.h (host side: sf_hip_tracks.hip): the regions of sf_regions.h followed from
// frame to frame. The labelling itself is the seven launches of sf_hip_regions.hip, unchanged; behind them run three kernels,
// one launch each on the handle's stream with entry = blockIdx.y (the assignment: blockIdx.x). What needs a grid-wide order
// is a launch boundary, NO WORKGROUP EVER WAITS FOR ANOTHER, and every loop is bounded by a count known at launch.
//
//   1 sft_overlap_kernel  the hot path. Lanes run down v, along memory: 8 bytes per previous pixel (clipped label, depth); for
//                         tracked pixels only, the warp and a gather of label and depth at the target. Equal (t, k) pairs
//                         are combined inside the wave before any atomic (one ballot per distinct pair: neighbouring lanes
//                         nearly always hit the same pair), then added to a table of the workgroup in LDS while
//                         K_prev * K <= SFT_LDS_PAIRS (16 KB), which is flushed once with global atomics; larger tables
//                         take the integer atomics straight on the global O. Both paths add the same integers.
//   2 sft_assign_kernel   one workgroup per entry: the loop of sf_track_assign.h (at most min(K_prev, K) rounds of a
//                         block-wide arg-max), the new ids, the row table of the slot, the head of every track record and
//                         the summary. It reads the slot's rows into LDS before it writes them.
//   3 sft_commit_kernel   one pass over the current frame: world-frame quantised sums and boxes per row (a wave-level
//                         reduction, then one set of atomics per wave and row), the id image, the slot's clipped label
//                         image, depth and camera. The slot's images are written only here, two launches behind the only
//                         kernel that reads them.
#pragma once
#include "../../include/sf_tracks.h"
#include "sf_device_common.h"
#include "sf_track_assign.h"

#define SFT_NT 256          // threads of every kernel in here
#define SFT_PB 2048         // previous pixels per workgroup of the overlap kernel: SFT_NT lanes x 8, strided by SFT_NT
#define SFT_LDS_PAIRS 4096  // the LDS budget of the overlap table: 4096 int32 = 16 KB of the workgroup's 64 KB

// The head of a slot's state (64 bytes); the camera, the rows and the two images follow at the offsets of TkLayout.
struct TkSlotHead {
    int frames, given, k_prev, pad[13];  // given: ids handed out so far, next_id - 1 (a zero-filled slot is a fresh slot)
};

// Where the pieces of a slot lie from its first byte (the same for every slot of a tracker), and the size of a slot.
struct TkLayout {
    size_t o_cam, o_id, o_birth, o_count, o_labels, o_depth, stride;
};

struct TkArgs {
    const float *depth;   // the current frame, rows x cols column-major
    const int *labels;    // its label image (all R numbers), in the tracker's scratch
    int *ids;             // the id image of the entry, or null
    unsigned char *slot;  // the slot's state
    float D[16];          // sft_relative(previous pose, current pose)
    sft_camera cam;       // the current camera
    float cx0, cy0, fx0, fy0;  // the previous camera's intrinsics
    float dz_abs, dz_rel;
    int has_prev, min_overlap, min_share, use_gate;
};

__device__ __forceinline__ int tk_wave_min(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = min(v, __shfl_xor(v, d, 64));
    return v;
}
__device__ __forceinline__ int tk_wave_max(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
    return v;
}
// row i of a 4 x 4 column-major transform applied to a point, in the header's order
__device__ __forceinline__ float tk_row(const float *T, int i, float x, float y, float z) {
    const float a = T[i] * x;
    const float b = T[i + 4] * y;
    const float c = T[i + 8] * z;
    const float ab = a + b;
    const float abc = ab + c;
    return abc + T[i + 12];
}

// ---- 1. overlap ---------------------------------------------------------------------------------------------------------
// One pair per lane (key = (t - 1) << 8 | (k - 1), or -1): the wave adds each distinct pair once. Every trip retires the lanes of
// one pair, so there are at most 64 trips.
__device__ __forceinline__ void tk_count_pairs(int key, bool lds, int *tab, int *O, int K, int M) {
    const int lane = (int)threadIdx.x & 63;
    unsigned long long todo = __ballot(key >= 0);
    for (int trip = 0; trip < 64; trip++) {
        if (todo == 0) break;  // (the whole wave)
        const int leader = __ffsll((long long)todo) - 1;
        const int key0 = __shfl(key, leader, 64);
        const unsigned long long same = __ballot(key == key0);
        if (lane == leader) {
            const int t0 = key0 >> 8, k0 = key0 & 255, count = __popcll(same);
            if (lds) atomicAdd(&tab[t0 * K + k0], count);
            else atomicAdd(&O[t0 * M + k0], count);
        }
        todo &= ~same;
    }
}

__global__ __launch_bounds__(SFT_NT) void sft_overlap_kernel(const TkArgs *args, TkLayout lay, int rows, int cols, int M, const sfr_summary *rsum, int *O_all,
                                                             sft_summary *sums) {
    __shared__ int tab[SFT_LDS_PAIRS];
    const TkArgs &a = args[blockIdx.y];
    if (!a.has_prev) return;  // (the whole workgroup, like every return before the barriers below)
    const int k_prev = ((const TkSlotHead *)a.slot)->k_prev;
    if (k_prev == 0) return;
    const int K = rsum[blockIdx.y].n_written;  // min(R, M)
    const int pairs = k_prev * K;
    const bool lds = pairs <= SFT_LDS_PAIRS;
    const int tid = threadIdx.x, px = rows * cols;
    int *O = O_all + (size_t)blockIdx.y * M * M;
    if (lds)
        for (int i = tid; i < pairs; i += SFT_NT) tab[i] = 0;
    __syncthreads();
    const int *lab0 = (const int *)(a.slot + lay.o_labels);
    const float *z0 = (const float *)(a.slot + lay.o_depth);
    const float fcols = (float)cols, frows = (float)rows;
    int warped = 0;
#pragma unroll 2
    for (int j = 0; j < SFT_PB / SFT_NT; j++) {
        const int i = (int)blockIdx.x * SFT_PB + j * SFT_NT + tid;
        int key = -1;
        const int t = i < px ? lab0[i] : 0;
        if (t > 0) {
            const float z = z0[i];
            const int u = i / rows, v = i - u * rows;
            const float du = (float)u - a.cx0, dv = (float)v - a.cy0;
            const float xu = du * z, yv = dv * z;
            const float X = xu / a.fx0, Y = yv / a.fy0;
            const float hx = tk_row(a.D, 0, X, Y, z), hy = tk_row(a.D, 1, X, Y, z), hz = tk_row(a.D, 2, X, Y, z);
            if (hz > 0.f) {
                const float nu = a.cam.fx * hx, nv = a.cam.fy * hy;
                const float qu = nu / hz, qv = nv / hz;
                const float uf = qu + a.cam.cx, vf = qv + a.cam.cy;
                const float su = uf + 0.5f, sv = vf + 0.5f;
                const float ui = floorf(su), vi = floorf(sv);
                if (ui >= 0.f && ui < fcols && vi >= 0.f && vi < frows) {
                    warped++;
                    const int at = (int)vi + (int)ui * rows;
                    const int k = a.labels[at];
                    if (k >= 1 && k <= K) {
                        bool counts = true;
                        if (a.use_gate) {
                            const float zc = a.depth[at];
                            const float diff = hz - zc;
                            const float nearer = fminf(hz, zc);
                            const float rel = a.dz_rel * nearer;
                            const float bound = a.dz_abs + rel;
                            counts = fabsf(diff) <= bound;
                        }
                        if (counts) key = ((t - 1) << 8) | (k - 1);
                    }
                }
            }
        }
        tk_count_pairs(key, lds, tab, O, K, M);
    }
    warped = wave_sum(warped);
    if ((tid & 63) == 0 && warped) atomicAdd(&sums[blockIdx.y].n_warped, warped);
    if (lds) {
        __syncthreads();
        for (int i = tid; i < pairs; i += SFT_NT) {
            const int c = tab[i];
            if (c) {
                const int t0 = i / K;
                atomicAdd(&O[t0 * M + (i - t0 * K)], c);
            }
        }
    }
}

// ---- 2. assignment ------------------------------------------------------------------------------------------------------
struct TkTeam {
    unsigned long long *red;  // SFT_NT / 64 words of LDS
    __device__ int lanes() const { return SFT_NT; }
    __device__ int lane() const { return (int)threadIdx.x; }
    __device__ void sync() const { __syncthreads(); }
    __device__ uint64_t max_of(uint64_t v) const {
        unsigned long long w = v;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const unsigned long long o = __shfl_xor(w, d, 64);
            w = o > w ? o : w;
        }
        if (((int)threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
        __syncthreads();
        unsigned long long best = red[0];
#pragma unroll
        for (int k = 1; k < SFT_NT / 64; k++) best = red[k] > best ? red[k] : best;
        __syncthreads();  // (before the next round writes red)
        return best;
    }
};

__global__ __launch_bounds__(SFT_NT) void sft_assign_kernel(const TkArgs *args, TkLayout lay, int M, const sfr_summary *rsum, const sfr_region *rreg, const int *O_all,
                                                            sft_summary *sums, sft_track *tracks) {
    __shared__ int32_t n_prev[SFT_MAX_TRACKS], n_cur[SFT_MAX_TRACKS], prev_of_cur[SFT_MAX_TRACKS], cur_of_prev[SFT_MAX_TRACKS];
    __shared__ int32_t id_prev[SFT_MAX_TRACKS], birth_prev[SFT_MAX_TRACKS], id_new[SFT_MAX_TRACKS];
    __shared__ unsigned long long red[SFT_NT / 64];
    __shared__ int next_after;
    const int q = blockIdx.x, tid = threadIdx.x;
    const TkArgs &a = args[q];
    TkSlotHead *head = (TkSlotHead *)a.slot;
    int *row_id = (int *)(a.slot + lay.o_id), *row_birth = (int *)(a.slot + lay.o_birth), *row_count = (int *)(a.slot + lay.o_count);
    const int k_prev = a.has_prev ? head->k_prev : 0, frames = head->frames, next_id = head->given + 1;
    const int R = rsum[q].n_regions, K = rsum[q].n_written;
    const sfr_region *reg = rreg + (size_t)q * M;
    const int *O = O_all + (size_t)q * M * M;
    if (tid < k_prev) {
        id_prev[tid] = row_id[tid];
        birth_prev[tid] = row_birth[tid];
        n_prev[tid] = row_count[tid];
    }
    if (tid < K) n_cur[tid] = reg[tid].n;
    __syncthreads();
    TkTeam team;
    team.red = red;
    const int matched = sft_assign_rounds(team, k_prev, K, O, M, n_prev, n_cur, a.min_overlap, a.min_share, prev_of_cur, cur_of_prev);
    if (tid == 0) {  // births in ascending k: at most M steps
        int id = next_id;
        for (int c = 0; c < K; c++)
            if (prev_of_cur[c] == 0) id_new[c] = id++;
        next_after = id;
    }
    __syncthreads();
    sft_track *rec = tracks + (size_t)q * M;
    if (tid < K) {
        const int t = prev_of_cur[tid];
        const sfr_region r = reg[tid];
        sft_track o;
        o.id = t ? id_prev[t - 1] : id_new[tid];
        o.region = tid + 1;
        o.prev_region = t;
        o.birth_frame = t ? birth_prev[t - 1] : frames;
        o.age = frames - o.birth_frame;
        o.overlap = t ? O[(t - 1) * M + tid] : 0;
        o.n = r.n; o.first = r.first; o.v_min = r.v_min; o.v_max = r.v_max; o.u_min = r.u_min; o.u_max = r.u_max; o.z_min = r.z_min; o.z_max = r.z_max;
        o.sum_v = r.sum_v; o.sum_u = r.sum_u; o.sum_z = r.sum_z; o.sum_b = r.sum_b;
        for (int j = 0; j < 3; j++) {
            o.qmin[j] = 0x7fffffff;
            o.qmax[j] = -0x7fffffff - 1;
            o.sum_q[j] = 0;
        }
        rec[tid] = o;
        row_id[tid] = o.id;  // (every lane read its rows into LDS before the first barrier)
        row_birth[tid] = o.birth_frame;
        row_count[tid] = r.n;
    }
    constexpr int WORDS = (int)(sizeof(sft_track) / sizeof(long long));
    long long *w = (long long *)rec;
    for (int i = K * WORDS + tid; i < M * WORDS; i += SFT_NT) w[i] = 0;
    if (tid == 0) {
        head->frames = frames + 1;
        head->given = next_after - 1;
        head->k_prev = K;
        sft_summary *s = sums + q;  // (n_warped: the overlap kernel)
        s->n_regions = R;
        s->n_tracked = K;
        s->n_matched = matched;
        s->n_born = K - matched;
        s->n_ended = k_prev - matched;
        s->n_untracked = R - K;
        s->next_id = next_after;
    }
}

// ---- 3. world statistics and commit -------------------------------------------------------------------------------------
__global__ __launch_bounds__(SFT_NT) void sft_commit_kernel(const TkArgs *args, TkLayout lay, int rows, int cols, int M, const sfr_summary *rsum, sft_track *tracks) {
    const int q = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const TkArgs &a = args[q];
    const int K = rsum[q].n_written, px = rows * cols;
    sft_track *rec = tracks + (size_t)q * M;
    const int i = (int)blockIdx.x * SFT_NT + tid;
    if (blockIdx.x == 0 && tid < (int)(sizeof(sft_camera) / 4)) ((float *)(a.slot + lay.o_cam))[tid] = ((const float *)&a.cam)[tid];
    int k = 0, qv[3] = {0, 0, 0};
    if (i < px) {
        const int lab = a.labels[i];
        const float z = a.depth[i];
        k = (lab >= 1 && lab <= K) ? lab : 0;
        ((int *)(a.slot + lay.o_labels))[i] = k;
        ((float *)(a.slot + lay.o_depth))[i] = z;
        if (a.ids) a.ids[i] = k ? rec[k - 1].id : 0;
        if (k) {
            const int u = i / rows, v = i - u * rows;
            const float du = (float)u - a.cam.cx, dv = (float)v - a.cam.cy;
            const float xu = du * z, yv = dv * z;
            const float X = xu / a.cam.fx, Y = yv / a.cam.fy;
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const float W = tk_row(a.cam.pose, j, X, Y, z);
                const float lo = fmaxf(W, -2048.f);
                const float cl = fminf(lo, 2048.f);
                qv[j] = (int)rintf(cl * 1024.f);
            }
        }
    }
    // one set of atomics per wave and row: every trip retires the lanes of one row, so there are at most 64 trips
    unsigned long long todo = __ballot(k > 0);
    for (int trip = 0; trip < 64; trip++) {
        if (todo == 0) break;  // (the whole wave)
        const int leader = __ffsll((long long)todo) - 1;
        const int k0 = __shfl(k, leader, 64);
        const bool join = k == k0;
        int lo[3], hi[3];
        long long sum[3];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            lo[j] = tk_wave_min(join ? qv[j] : 0x7fffffff);
            hi[j] = tk_wave_max(join ? qv[j] : -0x7fffffff - 1);
            sum[j] = wave_sum(join ? (long long)qv[j] : 0ll);
        }
        if (lane == leader) {
            sft_track *r = rec + (k0 - 1);
#pragma unroll
            for (int j = 0; j < 3; j++) {
                atomicMin(&r->qmin[j], lo[j]);
                atomicMax(&r->qmax[j], hi[j]);
                atomicAdd((unsigned long long *)&r->sum_q[j], (unsigned long long)sum[j]);
            }
        }
        todo &= ~__ballot(join);
    }
}

// ---- reset --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SFT_NT) void sft_reset_kernel(unsigned char *state, TkLayout lay, const int *slots, int n, int restart_ids) {
    const int i = (int)blockIdx.x * SFT_NT + (int)threadIdx.x;
    if (i >= n) return;
    TkSlotHead *head = (TkSlotHead *)(state + (size_t)slots[i] * lay.stride);
    head->k_prev = 0;
    if (restart_ids) {
        head->frames = 0;
        head->given = 0;
    }
}
