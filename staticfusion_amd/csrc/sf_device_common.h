// sf_device_common.h — shared definitions of the gfx950 solver kernels.
//
// Execution model: ONE WORKGROUP PER STREAM (independent RGB-D sequence).  A
// workgroup of SF_NT threads (8 wave64) owns a stream for a whole stage sequence; every
// "grid-wide" dependency of the reference algorithm (global max of the pre-weights, the 21+6
// normal-equation reduction, per-label residual sums, IRLS / level convergence tests) becomes a
// workgroup-local reduction through wave shuffles + LDS, so there is no inter-workgroup
// communication, no host round trip and no launch inside the coarse-to-fine loop.  256 CUs x 2
// resident workgroups keep 512 streams in flight; the streamed records of one stream (3.5 MB at
// QVGA) do not fit on chip, so the IRLS passes are HBM-bound.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sf.h"
#include "sf_build_config.h"  // (first: the build axes, their defaults and the combinations that are built)

// The frame kernels are compiled twice (sf_frame_kernels.hip): SF_NT = 256, four workgroups per CU -- the throughput
// variant, thousands of streams -- and SF_NT = 1024, one 16-wave workgroup per CU and stream -- the latency variant,
// up to a few hundred streams. The host (sf_hip.hip) picks one per handle.
#define SF_NW (SF_NT / 64) // waves per workgroup
#define SF_NC SF_NUM_CLUSTERS
#define SF_INVALID_LABEL 255

// in-kernel stage timers (wall_clock64, 100 MHz), accumulated per stream
enum {
    PF_PYR_OLD = 0, PF_PYR_NEW, PF_KMEANS, PF_WARP, PF_LINEARISE, PF_IRLS_INIT, PF_PASS1, PF_SOLVE6, PF_PASS2,
    PF_TAIL, PF_FILTER, PF_RESIDUALS, PF_SEGM_HIST, PF_TOTAL,
    PF_KM_INIT, PF_KM_SORT, PF_KM_ASSIGN, PF_KM_PARTITION, PF_KM_SUM, PF_KM_LABEL0, PF_KM_CONN_PYR,
    PF_SPLAT_REPLAYS = 24,  // not a timer (a slot of its own: 21..23 are shared by the profiling builds and the isolated-pass kernel): warp tiles replayed for targets outside their window (sf_splat.h: tiled_splat, lazy mode)
    PF_ORDERED_FALLBACKS = 25,  // not a timer: levels whose ordered tile splat gave up (a tap outside its window) and took the per-cell lists
    PF_SHADER_CYCLES = 26,  // the shader clock's cycles (clock64) over the same intervals as PF_TOTAL: cycles / ticks x 100 MHz = the clock the stream-frames ran at
    SF_PROF_SLOTS = 32
};

// record planes written by the linearisation and streamed by the IRLS passes.  Only what cannot be
// recomputed per pixel is stored: the warped depth, the four stencil gradients and the intensity
// difference (24 B) + one label byte; the passes also read the NEW depth from the pyramid (4 B).
// Inter depth / x / y, ddt and both pre-weights are recomputed with the reference's float
// expressions (bit-identical), which cuts the streamed bytes from 45 to 29 per pixel and pass.
enum { R_DW = 0, R_DCU, R_DCV, R_DCT, R_DDU, R_DDV, R_COUNT };

// stage mask bits of the frame kernel
enum {
    ST_PYR_OLD = 1,      // createImagePyramid(true)
    ST_PYR_NEW = 2,      // createImagePyramid(false)
    ST_KMEANS = 4,       // kMeans3DCoord + createClustersPyramidUsingKMeans
    ST_SOLVE = 8,        // coarse-to-fine loop of runSolver
    ST_RESIDUALS = 16,   // computeResidualsAgainstPreviousImage(index)
    ST_SEGM_IMAGE = 32,  // buildSegmImage
    ST_PUSH_HISTORY = 64, // ring[im_count % 5] = current
    ST_AUTO_RESIDUALS = 128, // several frames per launch: ST_RESIDUALS from the frame with im_count >= SF_HISTORY on
    ST_SOLVER_FORWARD = 256  // test and A/B support: IRLS pass 2 walks its records upwards like pass 1 (sf_irls.h), not back down
};

// Several consecutive frames of every stream in ONE launch of the frame kernel (sf_process_frames /
// sf_process_sequence_frames_device): the queue then hands out (frame, stream) pairs, frame-major, and a workgroup starts
// frame k of a stream as soon as frame k - 1 of THAT stream is done -- no barrier over the batch between frames, so the
// workgroups never line up again (a launch per frame makes all of them start with the same HBM-bound stage and ends with
// a tail in which the streams that needed most iterations run alone).
struct FrameLaunch {
    int stage_mask, im_count, n_frames;
    int *frame_done;        // [batch] frames of THIS launch completed per stream (zeroed by the host); null for one frame
    const int *seq_index;   // [n_frames][batch] pool frame of (frame, stream), < 0: leave the stream's images alone; or null
    const float *pool_d, *pool_i;  // [pool frame][n0]
    float *traj;            // [n_frames][batch][16] T_odometry after every frame, or null
    unsigned spin_limit;    // polls a workgroup waits for the previous frame of its stream
    int flip_ok;            // sequences: swap the roles of the two pyramid buffers instead of copying prediction := current
    int pass_window_px;     // IRLS passes: the last pass_window_px pixels of every sweep are loaded with the default policy, the rest nt (sf_irls.h: pass_division)
    int debug_give_up;      // test support: frame k = debug_give_up of every third stream is given up as if its wait had run out (0: never)
};

// fixed-point scales of the order-independent accumulations
#define FIX_DEPTH 67108864.f        /* 2^26 : warp depth accumulators */
#define FIX_INTENS 268435456.f      /* 2^28 : warp intensity accumulators (44-bit field, see ACC_W_SHIFT) */
// An accumulator cell is two 64-bit words: sum(w * depth) in Q26, and sum(w) << 44 + sum(w * intensity) in Q28 --
// the integer weight sum (each weight <= 200) shares the intensity word, so a splat is two atomics and a cell is
// 16 bytes. The intensity field holds +-2^43: > 160 full-weight contributions of intensity 1 on ONE cell (a rigid
// warp between neighbouring frames produces < 10); sum(w) holds 2^20.
#define ACC_W_SHIFT 44
#define FIX_RES 4294967296.f        /* 2^32 : per-label residual / prior sums */

// Per-stream persistent state (global memory, one per stream).
struct StreamState {
    float T[16];            // T_odometry, column-major
    float twist[6];         // twist_odometry
    float twist_level[6];   // twist_level_odometry
    float twist_old[6];     // twist_odometry_old
    float est_cov[36];
    float b_segm[SF_NC];
    float b_prior[SF_NC];
    float lambda_t_w[SF_NC];
    float kmeans[3 * SF_NC];        // column-major 3 x 24
    uint32_t conn[SF_NC];           // connectivity bit rows
    float cluster_res[SF_NC];       // perClusterAverageResidual
    float hist_T[SF_HISTORY][16];   // odomBuffer
    float kb;
    int32_t last_level;             // image level of the last executed outer iteration
    int32_t last_first;             // 1 if that iteration ran on Warped := Pred (the first of a solve)
    uint32_t sync_epoch;            // cluster build: tag of the last rendezvous of this stream's workgroups (sf_cluster.h)
    int32_t last_slot;              // record slot of the last executed outer iteration (cluster build: may be a private one)
    int32_t flip;                   // 1: the stream's two pyramid buffers have swapped roles (pyr_plane): only INSIDE a launch of
                                    // several frames of a sequence (sf_frame_kernels.hip), 0 whenever the host looks
    // Only INSIDE a launch of several SEQUENCE frames (null whenever the host looks): level 0 of the [set][channel] image is the
    // pool frame at this address instead of the pyramid buffer's level 0 (pyr_level) -- the launch reads the new frame, and as the
    // next frame's prediction the previous one, where they lie in the caller's HBM pool instead of copying 16 B per pixel and frame
    const float *lvl0[2][2];
    int32_t sync_failed;            // cluster build, sticky: a rendezvous of this stream timed out (sf_cluster.h: cluster_fail). Its frames
                                    // report SF_STATUS_SYNC_TIMEOUT and leave the state untouched until sf_clear_sync_timeout
    float inv_max_c, inv_max_d;     // 1/max of the raw pre-weights of that iteration
    long long cum_frames, cum_irls, cum_outer, cum_pixel_iters;  // totals since sf_create
    long long prof[SF_PROF_SLOTS];  // cumulative 100 MHz ticks per stage (lane 0 of the workgroup)
};

// Geometry, parameters and buffer table of a handle: lives in device memory, read through
// scalar loads (uniform addresses).  Per-launch values (stage mask, frame index) are kernel arguments.
struct KArgs {
    // geometry
    int rows, cols, levels, batch;
    int lrows[SF_MAX_LEVELS], lcols[SF_MAX_LEVELS], loff[SF_MAX_LEVELS], ln[SF_MAX_LEVELS];
    int n_tot;  // sum of level sizes
    int n0;     // level-0 size
    // parameters
    sf_params p;
    float tan_half_fovh;  // tanf(0.5f*fovh), evaluated on the host like the reference does
    // buffers
    float *pyr_new[4];   // [ch][batch][n_tot]  depth, intensity (xx, yy are recomputed: level_coord(); entries 2, 3 are null)
    float *pyr_pred[4];
    float *dbg_warped[4];  // debug_planes only, else null
    float *dbg_inter[4];
    uint8_t *labels;     // [batch][n_tot]
    long long *acc_d;    // [batch][n0] warp accumulators
    long long *acc_i;    // packed: (sum w << ACC_W_SHIFT) + sum(w * intensity)
    float *rec[R_COUNT];  // [plane][batch][n0]
    uint8_t *rec_lab;     // [batch][n0]  label of a valid pixel, SF_INVALID_LABEL otherwise
    uint8_t *rec_null;    // [batch][n0]  Null mask of the last linearisation
    const uint8_t *km_seed_lab;  // [ln[1]] label of the nearest K-means seed of every level-1 pixel (image-size constant, built at sf_create)
    float *hist_d, *hist_i;  // [SF_HISTORY][batch][n0]
    float *b_img;            // [batch][n0]
    StreamState *state;      // [batch]
    sf_frame_stats *stats;   // [batch]
    int *queue;              // work-queue counter (zeroed before every launch)
    const int *order;        // null, or the order in which the queue hands out the streams (longest expected first)
    // cluster build (sf_cluster.h): workgroups per stream; granules [batch][2][cluster_g][SF_SYNC_WORDS]. The record /
    // accumulator arrays then hold batch * (1 + cluster_g) slots of n0 pixels: slot b is stream b's shared one, slot
    // batch + b * cluster_g + r the private one of its workgroup r (coarse levels run redundantly per workgroup)
    int cluster_g;
    unsigned long long *sync;
    // test support (sf_debug_stall_rank): the workgroup of this rank of every stream idles `debug_stall_ticks` of the
    // 100 MHz clock before its first stage -- a late workgroup, as a co-running kernel causes -- and the rendezvous give up
    // after `sync_spin_limit` polls (0: SF_SYNC_SPIN_LIMIT)
    int debug_stall_rank;
    unsigned debug_stall_ticks, sync_spin_limit;
    // reference-order build only (sf_reforder.h; null otherwise): per record slot, RO_LIST_K source-pixel indices per cell
    int *ro_list;
    int ro_blocks;  // product builds: blocks of SF_ORDERED_SPLAT_MAX_PIXELS * RO_LIST_K indices in ro_list (sf_reforder.h: ro_list_of)
};

// The two pyramid buffers of a stream: set 0 = new (depthCurrent and its levels), set 1 = Pred. When consecutive frames
// of a SEQUENCE are solved inside one launch, the prediction of frame k + 1 is the current image of frame k and its pyramid
// is the pyramid frame k built: the buffers swap roles (StreamState::flip) instead of 0.6 MB being copied and a pyramid
// rebuilt bit for bit. Every stage takes its base pointers here.
__device__ __forceinline__ float *pyr_plane(const KArgs &a, int b, int set, int ch) {
    // an atomic (vector-memory) load: never the scalar data cache, which this workgroup's own store would not update
    const int f = __builtin_amdgcn_readfirstlane(__hip_atomic_load(&a.state[b].flip, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
    float *const *tab = ((set ^ f) & 1) ? a.pyr_pred : a.pyr_new;
    return tab[ch] + (size_t)b * a.n_tot;
}
// Level L of the [set][ch] image for READING: the pyramid buffer's, or -- level 0 inside a launch of sequence frames -- the pool
// frame the stream's StreamState::lvl0 names (read like `flip`: a vector-memory load, uniform, moved to SGPRs by as_global)
__device__ __forceinline__ const float *pyr_level(const KArgs &a, int b, int set, int ch, int L) {
    const float *p = pyr_plane(a, b, set, ch) + a.loff[L];
    if (L == 0) {
        const unsigned long long o = __hip_atomic_load((const unsigned long long *)&a.state[b].lvl0[set][ch], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)o), hi = __builtin_amdgcn_readfirstlane((unsigned)(o >> 32));
        if (lo | hi) p = (const float *)(((unsigned long long)hi << 32) | lo);
    }
    return p;
}

// ---------------------------------------------------------------------------------------------
//  wave / workgroup reductions (deterministic: fixed shuffle tree, fixed wave order)
// ---------------------------------------------------------------------------------------------
// Wave reductions on the DPP network (row_shr 1/2/4/8 inside each row of 16 lanes, then row_bcast15 /
// row_bcast31 across rows: an inclusive scan whose last lane holds the total) instead of ds_bpermute
// shuffles: VALU-speed cross-lane moves, no trip through the LDS crossbar.  The association order is
// fixed, so the sums stay deterministic.  Every lane returns the total (broadcast from lane 63).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_i32(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xf, false);
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_f64(double v) {
    const long long b = __double_as_longlong(v);
    const int lo = dpp_i32<CTRL, ROW_MASK>((int)(b & 0xffffffffll)), hi = dpp_i32<CTRL, ROW_MASK>((int)(b >> 32));
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ long long dpp_i64(long long b) {
    const int lo = dpp_i32<CTRL, ROW_MASK>((int)(b & 0xffffffffll)), hi = dpp_i32<CTRL, ROW_MASK>((int)(b >> 32));
    return ((long long)hi << 32) | (unsigned)lo;
}
#define SF_DPP_REDUCE(v, MOVE, OP)         \
    v = OP(v, (MOVE<0x111, 0xf>(v)));      \
    v = OP(v, (MOVE<0x112, 0xf>(v)));      \
    v = OP(v, (MOVE<0x114, 0xf>(v)));      \
    v = OP(v, (MOVE<0x118, 0xf>(v)));      \
    v = OP(v, (MOVE<0x142, 0xa>(v)));      \
    v = OP(v, (MOVE<0x143, 0xc>(v)));
template <class T>
__device__ __forceinline__ T sf_op_add(T a, T b) { return a + b; }
__device__ __forceinline__ int sf_op_maxi(int a, int b) { return a > b ? a : b; }
__device__ __forceinline__ int sf_op_ori(int a, int b) { return a | b; }

__device__ __forceinline__ double wave_sum_f64(double v) {
    SF_DPP_REDUCE(v, dpp_f64, sf_op_add)
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), 63), hi = __builtin_amdgcn_readlane((int)(b >> 32), 63);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
__device__ __forceinline__ long long wave_sum_i64(long long v) {
    SF_DPP_REDUCE(v, dpp_i64, sf_op_add)
    const int lo = __builtin_amdgcn_readlane((int)(v & 0xffffffffll), 63), hi = __builtin_amdgcn_readlane((int)(v >> 32), 63);
    return ((long long)hi << 32) | (unsigned)lo;
}
__device__ __forceinline__ int wave_sum_i32(int v) {
    SF_DPP_REDUCE(v, dpp_i32, sf_op_add)
    return __builtin_amdgcn_readlane(v, 63);
}
// maximum of non-negative floats (identity 0 shifts in at the row edges)
__device__ __forceinline__ float wave_max_f32(float v) {
    int b = __float_as_int(v);  // non-negative floats order like their bit patterns
    SF_DPP_REDUCE(b, dpp_i32, sf_op_maxi)
    return __int_as_float(__builtin_amdgcn_readlane(b, 63));
}
// The integer wave sums of the companion kernels (sf_p2p_device.h, sf_bodies.h, sf_score.h, sf_closure.h, sf_tracks.h,
// sf_regions.h): a butterfly of shuffles, every lane gets the total. Integers: the order of the additions does not show.
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// Exclusive scan of block_counts[0 .. n_blocks) in place by ONE 1024-thread workgroup, 1024 counts per trip; thread 0 gets the
// total. The scan stage of the ordered compactions (sf_fusion.h: clean; sf_map_window.h: partition).
__device__ __forceinline__ int block_counts_scan(int *block_counts, int n_blocks) {
    __shared__ int wsum[16];
    __shared__ int base;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) base = 0;
    __syncthreads();
    for (int c0 = 0; c0 < n_blocks; c0 += 1024) {
        const int idx = c0 + tid;
        const int v = idx < n_blocks ? block_counts[idx] : 0;
        int incl = v;  // inclusive scan within the wave (DPP-free, shuffle based: not a hot loop)
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(incl, off, 64);
            if (lane >= off) incl += o;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int off = base;
        for (int w = 0; w < wave; w++) off += wsum[w];
        if (idx < n_blocks) block_counts[idx] = off + incl - v;
        __syncthreads();
        if (tid == 0) {
            int t = 0;
            for (int w = 0; w < 16; w++) t += wsum[w];
            base += t;
        }
        __syncthreads();
    }
    return base;
}

// x86 cvttss2si semantics of the reference's int(float) (reference FrontEnd.cpp:819-820): NaN and
// out-of-range -> INT_MIN.  (v_cvt_i32_f32 would saturate and turn NaN into 0, which the
// reference's `uwarp >= 0` test would then ACCEPT.)
__device__ __forceinline__ int cvt_trunc_x86(float x) {
    if (!(x > -2147483648.f && x < 2147483648.f)) return (int)0x80000000;
    return (int)x;
}

// Buffer pointers come out of the KArgs table as generic pointers; every stage casts them to the
// GLOBAL address space so that loads / stores / atomics compile to global_* instructions (vmcnt only).
// With flat_* accesses every LDS wait also drains the outstanding global loads, which serialises
// prefetched loads behind the first LDS access.
// LDS: the workgroup's shared structs are passed to the (separately compiled) stage functions as
// references qualified with the LOCAL address space, so that their members are accessed with ds_*
// instructions (a plain reference is a generic pointer: every access becomes a flat_* instruction
// that waits on both memory counters).
#define LDS __attribute__((address_space(3)))
typedef float __attribute__((ext_vector_type(2))) vfloat2;  // plain vector types: usable in any address space
typedef float __attribute__((ext_vector_type(4))) vfloat4;
template <class T>
__device__ __forceinline__ void lds_add(LDS T *p, T v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
template <class T>
__device__ __forceinline__ void lds_min(LDS T *p, T v) {
    __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
template <class T>
__device__ __forceinline__ void lds_or(LDS T *p, T v) {
    __hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// a pointer that is the same in every lane, moved to an SGPR pair (arguments of the __noinline__
// stage functions arrive in VGPRs, which would force per-lane 64-bit address arithmetic)
template <class P>
__device__ __forceinline__ P uniform_ptr(P p) {
    const unsigned long long v = (unsigned long long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return (P)(((unsigned long long)hi << 32) | lo);
}
template <class T>
using gptr = __attribute__((address_space(1))) T *;
template <class T>
__device__ __forceinline__ gptr<T> as_global(T *p) {  // every base pointer of a stage is workgroup-uniform
    return uniform_ptr((gptr<T>)p);
}
// Element idx >= 0 of an array whose base is workgroup-uniform, addressed as SGPR base + 32-bit unsigned BYTE offset:
// the form the hardware takes directly (global_load ... v_off, s[base]). `p[idx]` with a signed int costs a sign extension
// and a 64-bit shift-add in VALU per access -- about 7 % of all VALU instructions of a frame before this was used.
// (The offset passes through an empty asm so that two accesses with the same index do not share one zero-extension node:
// instruction selection folds the extension into the addressing mode only when the access is its single user.)
__device__ __forceinline__ unsigned gbyte_off(int idx, unsigned elem) {
    unsigned off = (unsigned)idx * elem;
    asm("" : "+v"(off));
    return off;
}
template <class T>
__device__ __forceinline__ T gld(gptr<const T> p, int idx) {
    return *(gptr<const T>)((__attribute__((address_space(1))) const char *)p + gbyte_off(idx, (unsigned)sizeof(T)));
}
template <class T>
__device__ __forceinline__ T gld(gptr<T> p, int idx) {
    return *(gptr<const T>)((__attribute__((address_space(1))) const char *)p + gbyte_off(idx, (unsigned)sizeof(T)));
}
template <class T, class V>
__device__ __forceinline__ void gst(gptr<T> p, int idx, V v) {
    *(gptr<T>)((__attribute__((address_space(1))) char *)p + gbyte_off(idx, (unsigned)sizeof(T))) = (T)v;
}
// Scope of the warp / residual accumulator cells. In the one-workgroup-per-stream builds a stream's accumulators are
// touched by ONE workgroup between two kernel boundaries, so workgroup scope is all the coherence they need: the atomics
// then complete in this XCD's L2 and a cell is written back once, when its line is evicted. Agent scope (what a cluster
// of workgroups on different CUs needs) makes every atomic write through to the fabric: the zero store AND the sums both
// reached HBM, 34 bytes written per pixel and warp where 16 are needed (profiles/r02j_traffic_by_stage.txt).
#ifdef SF_CLUSTER
#define SF_ACC_SCOPE __HIP_MEMORY_SCOPE_AGENT
#else
#define SF_ACC_SCOPE __HIP_MEMORY_SCOPE_WORKGROUP
#endif
__device__ __forceinline__ void gatomic_add_at(gptr<long long> p, int idx, long long v) {
    __hip_atomic_fetch_add((gptr<long long>)((__attribute__((address_space(1))) char *)p + gbyte_off(idx, 8u)), v, __ATOMIC_RELAXED, SF_ACC_SCOPE);
}
template <class P>
__device__ __forceinline__ long long gld_agent_i64(P p, int idx) {  // load of a 64-bit accumulator cell at the accumulators' scope
    return __hip_atomic_load((gptr<const long long>)((__attribute__((address_space(1))) const char *)p + gbyte_off(idx, 8u)), __ATOMIC_RELAXED,
                             SF_ACC_SCOPE);
}
__device__ __forceinline__ void gatomic_add(gptr<long long> p, long long v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void gatomic_add(gptr<uint32_t> p, uint32_t v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// a value every lane holds identically (read from LDS / memory): move it to an SGPR
__device__ __forceinline__ float uniform_f(float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); }
__device__ __forceinline__ int uniform_i(int x) { return __builtin_amdgcn_readfirstlane(x); }

__device__ __forceinline__ float sqf(float x) { return x * x; }
// std::max / std::min of the reference (argument order matters for NaN)
__device__ __forceinline__ float std_max(float a, float b) { return (a < b) ? b : a; }
__device__ __forceinline__ float std_min(float a, float b) { return (b < a) ? b : a; }

// (long long)(y * scale) without the emulated float -> int64 conversion: v = y * scale (|v| <= 2^52 for every use here, the
// split works up to 2^57) is cut exactly into trunc(v / 2^26) and the remainder (both exact in float: v has 24 significant
// bits), each converted with the native 32-bit instruction. Truncation toward zero like the C conversion, bit for bit.
__device__ __forceinline__ long long to_fix(float x, float scale, float lim) {
    float y = x;
    if (!(y < lim)) y = lim;  // also catches NaN
    if (!(y > -lim)) y = -lim;
    const float v = y * scale;
    const float vh = truncf(v * (1.f / 67108864.f));
    const float vl = v - vh * 67108864.f;
    return (long long)(int)vh * 67108864ll + (long long)(int)vl;
}
// the same value for |lim * scale| < 2^31: one conversion (truncation toward zero, like the two-step form above)
__device__ __forceinline__ int to_fix_i32(float x, float scale, float lim) {
    float y = x;
    if (!(y < lim)) y = lim;
    if (!(y > -lim)) y = -lim;
    return (int)(y * scale);
}

// aggregate a per-lane 64-bit value into bins[label], one LDS atomic per distinct label per wave
__device__ __forceinline__ void wave_label_add_i64(bool active, int lab, long long v, LDS long long *bins, int lane) {
    unsigned long long rem = __ballot(active);
    while (rem) {
        const int src = __ffsll((long long)rem) - 1;
        const int l = __builtin_amdgcn_readlane(lab, src);
        const bool mine = active && lab == l;
        const unsigned long long m = __ballot(mine);
        const long long sum = wave_sum_i64(mine ? v : 0ll);
        if (lane == 0) lds_add(bins + l, sum);
        rem &= ~m;
    }
}
__device__ __forceinline__ void wave_label_count(bool active, int lab, LDS int *bins, int lane) {
    unsigned long long rem = __ballot(active);
    while (rem) {
        const int src = __ffsll((long long)rem) - 1;
        const int l = __builtin_amdgcn_readlane(lab, src);
        const unsigned long long m = __ballot(active && lab == l);
        if (lane == 0) lds_add(bins + l, (int)__popcll(m));
        rem &= ~m;
    }
}


// ---------------------------------------------------------------------------------------------
//  xx / yy of the pyramids (reference FrontEnd.cpp:385-386: xx = (inv_f_i (u - disp_u_i)) depth) are not
//  stored: every consumer has the depth and the pixel position and repeats this expression (same
//  operations, same bits), which saves 8 B per pixel on the pyramid write and on every read.
// ---------------------------------------------------------------------------------------------
struct LevelCoord {
    float inv_f_i, disp_u_i, disp_v_i, inv_rows;
    int rows_i;
};
__device__ __forceinline__ LevelCoord level_coord(const KArgs &a, int L) {
    LevelCoord c;
    const int rows_i = a.lrows[L], cols_i = a.lcols[L];
    c.inv_f_i = 2.f * a.tan_half_fovh / float(cols_i);
    c.disp_u_i = 0.5f * (cols_i - 1);
    c.disp_v_i = 0.5f * (rows_i - 1);
    c.inv_rows = 1.f / float(rows_i);
    c.rows_i = rows_i;
    return c;
}
__device__ __forceinline__ float coord_x(const LevelCoord &c, int u, float d) { return (c.inv_f_i * (float(u) - c.disp_u_i)) * d; }
__device__ __forceinline__ float coord_y(const LevelCoord &c, int v, float d) { return (c.inv_f_i * (float(v) - c.disp_v_i)) * d; }
// flat column-major index -> (u, v), exact (float reciprocal estimate + integer correction)
__device__ __forceinline__ void split_uv(const LevelCoord &c, int idx, int &u, int &v) {
    int q = (int)((float)idx * c.inv_rows);
    if (q * c.rows_i > idx) q--;
    if ((q + 1) * c.rows_i <= idx) q++;
    u = q;
    v = idx - q * c.rows_i;
}

// initializeKMeans (reference KMeans.cpp:63-101): the seed a level-1 pixel starts with is the nearest of 24 seed positions
// that depend on the image size only, in the reference's unsigned wrap-around arithmetic. One table per handle
// (KArgs::km_seed_lab, built by sf_seed_label_kernel at sf_create) instead of 24 squared distances per pixel and frame.
__device__ __forceinline__ unsigned km_seed_u(int cols_km, int l) { return (unsigned)roundf((unsigned)(l + 1) * (float(cols_km) / float(SF_NC + 1))); }
__device__ __forceinline__ unsigned km_seed_v(int rows_km, int l) { return (unsigned)roundf((unsigned)(l % 5 + 1) * (float(rows_km) / float(5 + 1))); }  // 5 = ceil(sqrt(24))
__device__ __forceinline__ unsigned km_nearest_seed(int rows_km, int cols_km, unsigned u, unsigned v) {
    unsigned lab = SF_NC, min_dist = 1000000u;
    for (unsigned l = 0; l < SF_NC; l++) {
        const unsigned dv = v - km_seed_v(rows_km, (int)l), du = u - km_seed_u(cols_km, (int)l);  // unsigned wrap-around as in the reference
        const unsigned q = dv * dv + du * du;
        if (q < min_dist) {
            lab = l;
            min_dist = q;
        }
    }
    return lab;
}

#define SF_LOAD_BATCH 4  // independent pixels whose loads are issued before any of them is consumed
