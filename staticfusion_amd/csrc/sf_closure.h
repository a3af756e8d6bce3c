// sf_closure.h — device code of include/sf_closure.h (host side: sf_hip_closure.hip): loop-closure constraints from two drawings of
// a place, many closures per call. The two maps of entry q have been drawn into key images by the drawing stage of the views
// (sfv_draw_keys: rays, clear, splat, large sprites) as views 2q (map_new from view_from) and 2q + 1 (map_old from view_to);
// the kernels here come behind it. Table entry blockIdx.y, the grid sized for the entry with the most samples, workgroups beyond
// their entry's samples leave at once.
//
// sfc_sample_kernel<false> (the counting pass) and <true> (the writing pass) are one text: one lane per sample reads its two
// keys, evaluates both winning fragments again from their keys, as sfs_score_kernel does, so zA / zO are the floats the depth
// image of a render holds, gathers rows 0 and 1 of the two surfels and calls the shared rule (sf_closure_rules.h). A lane emits
// 0, 1 or 2 records.
//   counting: the eight predicates are counted with wave ballots, the two sums are kept per lane in 64-bit integers, reduced
//     across the wave with shuffles, across the four waves through LDS, and added to the entry's accumulators with 64-bit
//     integer atomics: at most once per field per workgroup, not at all for a total of 0. The workgroup's number of records
//     goes to block_counts[blockIdx.x]. Integer sums: nothing depends on the order of arrival.
//   sfc_scan_kernel: block_counts_scan (sf_device_common.h, the one scan) turns the block counts of an entry into offsets.
//   writing (only after the host has the counts and has checked the capacity): the slot of a lane's first record is its rank
//     among the records of the lower lanes of its wave (two ballots), plus the records of the lower waves (LDS), plus the
//     workgroup's offset; whole 32-byte records go to out[first + slot], the LINK before the PIN. No atomics at all.
#pragma once
#include "sf_closure_rules.h"
#include "sf_view_common.h"

#define SFC_NT 256
#define SFC_FIELDS 10  // n_new, n_old, n_both, n_near, n_apart, n_links, n_pins, n_dropped, sum_dz, sum_shift

struct ClosureArgs {
    int stride, nx, n_samples;  // sample k is column s2 + (k % nx) * stride of row s2 + (k / nx) * stride
    int first;                  // the entry's first record in `out` (set by the host between the passes)
    int capacity;               // records `out` holds: the call's total (likewise); no record is written at or beyond it
    SfcRule rule;
    float pose_to[16];          // view_to.pose, column-major
    int *block_counts;          // [workgroups of the entry]: records per workgroup; after the scan their exclusive offsets
    int *total;                 // [1]: the entry's records, from the scan
    long long *acc;             // [SFC_FIELDS], zeroed before the counting pass
    SfcRecord *out;             // the records of the whole call (the writing pass)
};

// the winner of pixel (x, y) of a drawn view: floats 0 .. 7 of its surfel and the depth of its fragment; false: nothing drawn
__device__ __forceinline__ bool sfc_winner(const ViewArgs &a, int x, int y, float *q8, float &z) {
    const unsigned long long key = as_global(a.keys)[y + x * a.rows];
    if (key == SFV_EMPTY) return false;
    const int s = (int)(unsigned)(key & 0xffffffffull);
    PV3 h, n;
    float rad, depth;
    sfv_to_camera(a, s, h, n, rad);
    surfel_fragment(a, h, n, rad, x, y, z, depth);
    const auto rec = (gptr<const vfloat4>)surfel_record(a, s);
    const vfloat4 r0 = rec[0], r1 = rec[1];
    q8[0] = r0.x; q8[1] = r0.y; q8[2] = r0.z; q8[3] = r0.w;
    q8[4] = r1.x; q8[5] = r1.y; q8[6] = r1.z; q8[7] = r1.w;
    return true;
}

template <bool WRITE>
__global__ __launch_bounds__(SFC_NT) void sfc_sample_kernel(const ViewArgs *vtab, const ClosureArgs *ctab) {
    __shared__ long long part[SFC_NT / 64][SFC_FIELDS];
    __shared__ int wave_records[SFC_NT / 64];
    const ClosureArgs &c = ctab[blockIdx.y];
    const int k0 = (int)blockIdx.x * SFC_NT;
    if (k0 >= c.n_samples) return;  // a workgroup of a larger entry of the batch
    const ViewArgs &A = vtab[2 * blockIdx.y], &O = vtab[2 * blockIdx.y + 1];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int k = k0 + tid;
    bool has_a = false, has_o = false;
    float zA = 0.f, zO = 0.f;
    float sa[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, so[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    SfcRecord link, pin;
    long long q_dz = 0, q_shift = 0;
    int mask = 0;
    if (k < c.n_samples) {
        const int j = k / c.nx, i = k - j * c.nx;
        const int s2 = c.stride >> 1;
        const int x = s2 + i * c.stride, y = s2 + j * c.stride;  // inside the view: the host counted the samples (sfc_samples_along)
        has_a = sfc_winner(A, x, y, sa, zA);
        has_o = sfc_winner(O, x, y, so, zO);
        const SfcRule rule = c.rule;
        mask = sfc_link_core(has_a, sa, has_o, so, zA, zO, A.t_inv, c.pose_to, &rule, &link, &pin, &q_dz, &q_shift);
    }
    const bool is_link = (mask & SFC_BIT_LINK) != 0, is_pin = (mask & SFC_BIT_PIN) != 0;
    const unsigned long long b_link = __ballot(is_link), b_pin = __ballot(is_pin);
    if (lane == 0) wave_records[wave] = __popcll(b_link) + __popcll(b_pin);
    if (!WRITE) {
        long long cnt[8];  // wave-uniform
        cnt[0] = __popcll(__ballot(has_a));
        cnt[1] = __popcll(__ballot(has_o));
        cnt[2] = __popcll(__ballot((mask & SFC_BIT_BOTH) != 0));
        cnt[3] = __popcll(__ballot((mask & SFC_BIT_NEAR) != 0));
        cnt[4] = __popcll(__ballot((mask & SFC_BIT_APART) != 0));
        cnt[5] = __popcll(b_link);
        cnt[6] = __popcll(b_pin);
        cnt[7] = __popcll(__ballot((mask & SFC_BIT_LINK_DROPPED) != 0)) + __popcll(__ballot((mask & SFC_BIT_PIN_DROPPED) != 0));
        q_dz = wave_sum(q_dz);
        q_shift = wave_sum(q_shift);
        if (lane == 0) {
#pragma unroll
            for (int f = 0; f < 8; f++) part[wave][f] = cnt[f];
            part[wave][8] = q_dz;
            part[wave][9] = q_shift;
        }
        __syncthreads();
        if (tid < SFC_FIELDS) {
            long long v = 0;
#pragma unroll
            for (int w = 0; w < SFC_NT / 64; w++) v += part[w][tid];
            if (v) __hip_atomic_fetch_add(as_global(c.acc) + tid, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (tid == 0) {
            int t = 0;
#pragma unroll
            for (int w = 0; w < SFC_NT / 64; w++) t += wave_records[w];
            c.block_counts[blockIdx.x] = t;
        }
    } else {
        __syncthreads();
        int slot = c.first + c.block_counts[blockIdx.x];
        for (int w = 0; w < wave; w++) slot += wave_records[w];
        const unsigned long long lower = (1ull << lane) - 1ull;
        slot += __popcll(b_link & lower) + __popcll(b_pin & lower);
        vfloat4 *out = (vfloat4 *)c.out;  // 32-byte records at a 256-byte aligned base
        if (is_link && slot < c.capacity) {
            out[2 * (size_t)slot] = vfloat4{link.src[0], link.src[1], link.src[2], link.dst[0]};
            out[2 * (size_t)slot + 1] = vfloat4{link.dst[1], link.dst[2], link.time, link.weight};
            slot++;
        }
        if (is_pin && slot < c.capacity) {
            out[2 * (size_t)slot] = vfloat4{pin.src[0], pin.src[1], pin.src[2], pin.dst[0]};
            out[2 * (size_t)slot + 1] = vfloat4{pin.dst[1], pin.dst[2], pin.time, pin.weight};
        }
    }
}

// one workgroup per entry: the block counts become offsets, the total is the entry's number of records
__global__ __launch_bounds__(1024) void sfc_scan_kernel(const ClosureArgs *ctab) {
    const ClosureArgs &c = ctab[blockIdx.x];
    const int total = block_counts_scan(c.block_counts, (c.n_samples + SFC_NT - 1) / SFC_NT);
    if (threadIdx.x == 0) c.total[0] = total;
}
