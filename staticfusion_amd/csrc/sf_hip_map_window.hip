// sf_hip_map_window.hip — libsf_hip.so, the interface of include/sf_map_window.h (symbols sfw_*): a map is kept inside a
// budget by a stable partition of its surfel buffer into its idle second buffer (kernels: sf_map_window.h). Cull swaps the
// two buffers afterwards, extract copies the front part out, page-out copies the back part out and swaps. No frame kernel
// and no kernel of the fusion is involved; the scratch is the map's own clean-stage scratch (flags, block_counts), idle
// between two fuses. The join and the body maps launch the scan and the ordered write from here (sfw_launch_scan,
// sfw_launch_write), so the library holds those kernels once.
#include "../../include/sf_map_window.h"
#include "sf_host.h"
#include "sf_map_window.h"

#define SFW_VERSION 1
static_assert(sizeof(sfw_filter) == 32, "include/sf_map_window.h: sfw_filter is 32 bytes");

// Load policy of the record reads (A/B tooling, tools/map_window_bench.py): SF_WINDOW_POLICY=default | nt (the move pass reads
// non-temporally: its bytes are not read again) | nt2 (the predicate pass too). Unset: the measured choice, DESIGN.md section 18.
static int window_policy() {
    if (const char *v = std::getenv("SF_WINDOW_POLICY")) {
        if (!std::strcmp(v, "nt")) return 1;
        if (!std::strcmp(v, "nt2")) return 2;
        return 0;
    }
    return SFW_DEFAULT_POLICY;
}

static int check_filter(const sfw_filter *f) {
    if (!f) return fail(SF_ERR_ARG, "sfw: null filter");
    if (std::isnan(f->min_confidence) || std::isnan(f->radius) || std::isnan(f->centre[0]) || std::isnan(f->centre[1]) || std::isnan(f->centre[2]))
        return fail(SF_ERR_ARG, "sfw: NaN in min_confidence, radius or centre of a filter");
    return SF_OK;
}

// the checks every call makes before anything is launched
static int check_maps(const char *what, sf_handle *h, int n, sf_map *const *maps, const sfw_filter *filters) {
    for (int q = 0; q < n; q++) {
        if (int e = check_map(what, h, maps[q])) return e;
        if (int e = check_distinct(what, maps, q, "the same map twice in one batch")) return e;
        if (int e = check_filter(filters + q)) return e;
        if (((size_t)maps[q]->count + 63) / 64 * 8 > (size_t)maps[q]->capacity) return fail(SF_ERR_STATE, std::string(what) + ": map too small for its own scratch");
    }
    return SF_OK;
}

static void launch_write(sf_handle *h, const WindowArgs *tab, int n, int max_count) {
    if (!max_count) return;
    const dim3 grid((unsigned)((max_count + SFW_BLOCK - 1) / SFW_BLOCK), (unsigned)n);
    if (window_policy() >= 1)
        hipLaunchKernelGGL(sfw_write_kernel<true>, grid, dim3(SFW_BLOCK), 0, h->stream, tab);
    else
        hipLaunchKernelGGL(sfw_write_kernel<false>, grid, dim3(SFW_BLOCK), 0, h->stream, tab);
}

// ---- the scan and the ordered write for the join and the body maps (declared in sf_host.h)
void sfw_launch_scan(sf_handle *h, const WindowArgs *d_tab, int n) {
    hipLaunchKernelGGL(sfw_scan_kernel, dim3((unsigned)n), dim3(1024), 0, h->stream, d_tab);
}
void sfw_launch_write(sf_handle *h, const WindowArgs *d_tab, unsigned blocks, int n) {
    hipLaunchKernelGGL(sfw_write_kernel<false>, dim3(blocks, (unsigned)n), dim3(SFW_BLOCK), 0, h->stream, d_tab);
}

// Predicate pass and scan for n checked maps of h (with `write`: the move into buf[1] as well; move_rest: the surfels not
// selected are moved behind the selected ones, otherwise they are left out), then the counts read back: selected[q]. The
// table stays in h->tab_dev, so that a caller that decides on the counts can still launch the move.
static int partition(sf_handle *h, int n, sf_map *const *maps, const sfw_filter *filters, bool write, bool move_rest, int *selected,
                     const WindowArgs **d_tab, int *max_count_out) {
    HIP_TRY(hipSetDevice(h->device));
    if (int e = results_scratch(h, (size_t)n)) return e;
    std::vector<WindowArgs> tab((size_t)n);
    int max_count = 0;
    for (int q = 0; q < n; q++) {
        const sf_map *m = maps[q];
        const sfw_filter &f = filters[q];
        WindowArgs &a = tab[(size_t)q];
        a.src = m->buf[0];
        a.dst = m->buf[1];
        a.count = m->count;
        a.move_rest = move_rest;
        a.use_conf = f.min_confidence > 0.f;
        a.use_age = f.max_age >= 0;
        a.use_radius = f.radius > 0.f;
        a.invert = f.invert != 0;
        a.min_confidence = f.min_confidence;
        a.tick = float(m->tick);
        a.max_age = float(f.max_age);
        a.cx = f.centre[0]; a.cy = f.centre[1]; a.cz = f.centre[2];
        a.r2 = f.radius * f.radius;
        a.ballots = (unsigned long long *)m->flags;
        a.block_counts = m->block_counts;
        a.result = h->res_dev + (size_t)q * 8;
        max_count = std::max(max_count, m->count);
    }
    void *d = nullptr;
    if (int e = upload_table(h, tab.data(), tab.size() * sizeof(WindowArgs), &d)) return e;
    const WindowArgs *dev = (const WindowArgs *)d;
    if (max_count) {
        const dim3 grid((unsigned)((max_count + SFW_BLOCK - 1) / SFW_BLOCK), (unsigned)n);
        if (window_policy() >= 2)
            hipLaunchKernelGGL(sfw_flag_kernel<true>, grid, dim3(SFW_BLOCK), 0, h->stream, dev);
        else
            hipLaunchKernelGGL(sfw_flag_kernel<false>, grid, dim3(SFW_BLOCK), 0, h->stream, dev);
    }
    sfw_launch_scan(h, dev, n);
    if (write) launch_write(h, dev, n, max_count);
    HIP_TRY(hipGetLastError());
    std::vector<int> res((size_t)n * 8);
    if (int e = d2h(h, res.data(), h->res_dev, res.size() * sizeof(int))) return e;
    for (int q = 0; q < n; q++) {
        selected[q] = res[(size_t)q * 8];
        if (selected[q] < 0 || selected[q] > maps[q]->count) return fail(SF_ERR_DEVICE, "sfw: a count outside the map came back");
    }
    if (d_tab) *d_tab = dev;
    if (max_count_out) *max_count_out = max_count;
    return SF_OK;
}

// the partitioned buffer becomes the map: its first k surfels
static void adopt(sf_map *m, int k) {
    std::swap(m->buf[0], m->buf[1]);
    m->count = k;
    indices_moved(m);
}

extern "C" {

int sfw_version(void) { return SFW_VERSION; }
size_t sfw_filter_bytes(void) { return sizeof(sfw_filter); }
int sfw_check_filter(const sfw_filter *f) { return check_filter(f); }

int sfw_count_maps(sf_handle *h, int n, sf_map *const *maps, const sfw_filter *filters, int *selected) {
    if (!h || n < 0 || (n && (!maps || !filters || !selected))) return fail(SF_ERR_ARG, "sfw_count_maps: bad argument");
    if (n == 0) return SF_OK;
    if (int e = check_maps("sfw_count_maps", h, n, maps, filters)) return e;
    return partition(h, n, maps, filters, false, false, selected, nullptr, nullptr);
}

int sfw_cull_maps(sf_handle *h, int n, sf_map *const *maps, const sfw_filter *filters, int *kept) {
    if (!h || n < 0 || (n && (!maps || !filters || !kept))) return fail(SF_ERR_ARG, "sfw_cull_maps: bad argument");
    if (n == 0) return SF_OK;
    if (int e = check_maps("sfw_cull_maps", h, n, maps, filters)) return e;
    std::vector<int> k((size_t)n);
    if (int e = partition(h, n, maps, filters, true, false, k.data(), nullptr, nullptr)) return e;
    for (int q = 0; q < n; q++) {  // commit: only after the whole batch has run and its counts are back
        adopt(maps[q], k[(size_t)q]);
        kept[q] = k[(size_t)q];
    }
    return SF_OK;
}

// extract (page == 0): [0, k) of the partitioned buffer to the host; page out (page == 1): [k, count), then the buffer becomes the map
static int copy_out(const char *what, sf_map *m, const sfw_filter *f, float *surfels_out, int max_count, int *count, int page) {
    if (!m || !f || !count || max_count < 0 || (!surfels_out && max_count > 0)) return fail(SF_ERR_ARG, std::string(what) + ": bad argument");
    sf_handle *h = m->h;
    if (int e = check_maps(what, h, 1, &m, f)) return e;
    int k = 0, max_n = 0;
    const WindowArgs *tab = nullptr;
    if (int e = partition(h, 1, &m, f, false, page != 0, &k, &tab, &max_n)) return e;
    const int n_out = page ? m->count - k : k;
    *count = n_out;
    if (n_out > max_count) return fail(SF_ERR_ARG, std::string(what) + ": " + std::to_string(n_out) + " surfels, room for " + std::to_string(max_count));
    if (!page && n_out == 0) return SF_OK;  // nothing to copy and nothing to change
    launch_write(h, tab, 1, max_n);
    HIP_TRY(hipGetLastError());
    if (n_out) {
        if (int e = d2h(h, surfels_out, m->buf[1] + (size_t)(page ? k : 0) * 12, (size_t)n_out * 12 * sizeof(float))) return e;
    }
    if (page) adopt(m, k);
    return SF_OK;
}
int sfw_extract(sf_map *m, const sfw_filter *f, float *surfels_out, int max_count, int *count) {
    return copy_out("sfw_extract", m, f, surfels_out, max_count, count, 0);
}
int sfw_page_out(sf_map *m, const sfw_filter *f, float *surfels_out, int max_count, int *count) {
    return copy_out("sfw_page_out", m, f, surfels_out, max_count, count, 1);
}

int sfw_append(sf_map *m, const float *surfels, int count) {
    if (!m || count < 0 || (!surfels && count > 0)) return fail(SF_ERR_ARG, "sfw_append: bad argument");
    if (int e = check_part("sfw_append", m, "map")) return e;
    if ((long long)count + m->count > (long long)m->capacity) return fail(SF_ERR_STATE, "sfw_append: count + the map's count exceeds its capacity");
    HIP_TRY(hipSetDevice(m->h->device));
    if (count) {
        HIP_TRY(hipMemcpyAsync(m->buf[0] + (size_t)m->count * 12, surfels, (size_t)count * 12 * sizeof(float), hipMemcpyHostToDevice, m->h->stream));
        HIP_TRY(hipStreamSynchronize(m->h->stream));  // the host buffer is free again
    }
    m->count += count;
    indices_moved(m);
    return SF_OK;
}

}  // extern "C"
