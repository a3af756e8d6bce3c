// Does a non-temporal read stream leave default-policy lines in the memory-side cache (MALL, 256 MiB) alone? gfx950 probe behind
// the per-trip load policy of the IRLS passes: a table is read twice with default-policy loads; between
// the two reads a stream of another buffer is read with default-policy or with `nt` loads (8-byte loads, 8 in flight per lane:
// the record pairs of the passes). Reported: the rate of the SECOND table read, against two references -- the table read again
// at once (resident) and after 2 GiB of default-policy traffic (evicted). Kernel times are taken inside the kernel (100 MHz wall
// clock, first block in to last block out): a 32 MB read lasts ~5 us, less than a launch.
//   hipcc --offload-arch=gfx950 -O3 -o nt_retain nt_retain.hip && ./nt_retain [table MB ...]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
typedef float f2 __attribute__((ext_vector_type(2)));
typedef unsigned long long u64;

#define CHECK(e)                                                                              \
    do {                                                                                      \
        hipError_t e_ = (e);                                                                  \
        if (e_ != hipSuccess) {                                                               \
            fprintf(stderr, "%s: %s (line %d)\n", #e, hipGetErrorString(e_), __LINE__);       \
            exit(1);                                                                          \
        }                                                                                     \
    } while (0)

// every lane reads U strides per trip, all in flight before the first is used; a load past the end is skipped
template <bool NT, int U>
__global__ __launch_bounds__(256) void rd(const f2 *__restrict__ p, size_t n, float *out, u64 *span) {
    const u64 t0 = wall_clock64();
    float acc = 0.f;
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += U * stride) {
        f2 v[U];
#pragma unroll
        for (int k = 0; k < U; k++) {
            v[k] = f2{0.f, 0.f};
            if (i + k * stride < n) v[k] = NT ? __builtin_nontemporal_load(p + i + k * stride) : p[i + k * stride];
        }
#pragma unroll
        for (int k = 0; k < U; k++) acc += v[k].x + v[k].y;
    }
    if (acc == 12345.678f) out[0] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicMin(&span[0], t0);
        atomicMax(&span[1], (u64)wall_clock64());
    }
}

static int g_blocks;
static float *g_out;
static u64 *g_span;  // [0] first block in, [1] last block out (100 MHz ticks)

template <bool NT>
static void read_all(const void *buf, size_t bytes) {
    rd<NT, 8><<<g_blocks, 256>>>((const f2 *)buf, bytes / sizeof(f2), g_out, g_span);
}
// microseconds of one default-policy read of the table, timed inside the kernel
static double timed_table_read(const void *table, size_t bytes) {
    const u64 init[2] = {~0ull, 0ull};
    CHECK(hipMemcpy(g_span, init, sizeof(init), hipMemcpyHostToDevice));
    read_all<false>(table, bytes);
    CHECK(hipDeviceSynchronize());
    u64 s[2];
    CHECK(hipMemcpy(s, g_span, sizeof(s), hipMemcpyDeviceToHost));
    return (double)(s[1] - s[0]) * 0.01;
}
static double median(std::vector<double> v) {
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

int main(int argc, char **argv) {
    hipDeviceProp_t pr;
    CHECK(hipGetDeviceProperties(&pr, 0));
    g_blocks = pr.multiProcessorCount * 4;  // the throughput build's residency
    const size_t MiB = (size_t)1 << 20, stream_max = (size_t)1 << 30;
    std::vector<size_t> tables_mb = {32, 64, 128};
    if (argc > 1) {
        tables_mb.clear();
        for (int i = 1; i < argc; i++) tables_mb.push_back((size_t)atoi(argv[i]));
    }
    void *table, *stream;
    CHECK(hipMalloc(&table, 256 * MiB));
    CHECK(hipMalloc(&stream, stream_max));
    CHECK(hipMalloc(&g_out, 4));
    CHECK(hipMalloc(&g_span, 2 * sizeof(u64)));
    CHECK(hipMemset(table, 0, 256 * MiB));
    CHECK(hipMemset(stream, 0, stream_max));
    const int reps = 7;
    printf("%s, %d CUs, %d blocks of 256; 8-byte loads, 8 in flight per lane; median of %d, second table read in GB/s (us)\n", pr.gcnArchName,
           pr.multiProcessorCount, g_blocks, reps);
    for (size_t mb : tables_mb) {
        const size_t tb = std::min(mb * 1000000, 256 * MiB) & ~(size_t)7;
        std::vector<double> res, evi;
        for (int r = 0; r < reps; r++) {
            read_all<false>(table, tb);
            res.push_back(timed_table_read(table, tb));  // at once: as resident as this table gets
            read_all<false>(stream, stream_max);
            read_all<false>(stream, stream_max);
            evi.push_back(timed_table_read(table, tb));  // behind 2 GiB of default-policy reads: from HBM
        }
        printf("table %6.1f MB: read again at once %7.1f (%6.2f)   behind 2 GiB default %7.1f (%6.2f)\n", tb / 1e6, tb / median(res) / 1e3, median(res),
               tb / median(evi) / 1e3, median(evi));
        for (size_t smib : {128, 256, 512, 1024}) {
            const size_t sb = std::min(smib * MiB, stream_max);
            std::vector<double> d, n;
            for (int r = 0; r < reps; r++) {
                for (int nt = 0; nt < 2; nt++) {
                    // start from the same state both times: table out of the cache, then read once
                    read_all<false>(stream, stream_max);
                    read_all<false>(stream, stream_max);
                    read_all<false>(table, tb);
                    if (nt) read_all<true>(stream, sb);
                    else read_all<false>(stream, sb);
                    (nt ? n : d).push_back(timed_table_read(table, tb));
                }
            }
            printf("  stream %4zu MiB between:  default %7.1f (%6.2f)   nt %7.1f (%6.2f)\n", smib, tb / median(d) / 1e3, median(d), tb / median(n) / 1e3,
                   median(n));
        }
    }
    return 0;
}
