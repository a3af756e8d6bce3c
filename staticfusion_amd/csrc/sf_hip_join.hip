// sf_hip_join.hip — libsf_hip.so, the interface of include/sf_join.h (symbols sfj_*): maps thinned to one surfel per voxel and
// maps merged without storing a surface twice, many per call (kernels: sf_voxel_table.h, sf_join.h; key, rank and hash: sf_join_key.h). The
// voxel tables, the remembered slots, the ballots, the block counts, the counters and the two entry tables of a call lie in
// the call block sf_handle::join (sf_call_block.h: layout, growth and lifetime). A thin partitions a map into its idle second
// buffer like a cull, with the scan and the ordered write of the bounded maps (sfw_launch_scan / sfw_launch_write); a merge
// writes behind the destination's own surfels. One host synchronisation reads the counts; for a merge it lies before the
// move, because the capacity test needs them.
#include "../../include/sf_join.h"
#include "sf_host.h"
#include "sf_join.h"

#define SFJ_VERSION 1
static_assert(sizeof(sfj_params) == 32, "include/sf_join.h: sfj_params is 32 bytes");
static_assert(sizeof(sfj_counts) == 32, "include/sf_join.h: sfj_counts is 32 bytes");
static_assert(sizeof(sfj_counts) == SFJ_COUNT_WORDS * sizeof(int), "an entry's counters are read back as one record");

static int check_params(const sfj_params *p) {
    if (!p) return fail(SF_ERR_ARG, "sfj: null params");
    if (!(std::isfinite(p->cell) && p->cell > 0.f)) return fail(SF_ERR_ARG, "sfj: cell is finite and > 0");
    if (!std::isfinite(1.0f / p->cell)) return fail(SF_ERR_ARG, "sfj: 1 / cell is not finite");
    if (std::isnan(p->min_confidence)) return fail(SF_ERR_ARG, "sfj: NaN min_confidence");
    if (p->dry_run != 0 && p->dry_run != 1) return fail(SF_ERR_ARG, "sfj: dry_run is 0 or 1");
    return SF_OK;
}

struct JoinEntry {
    const sf_map *fill;  // fills the table: the map (thin), the destination (merge)
    const sf_map *src;   // examined: the map (thin), the source (merge)
    const float *T;      // merge: 16 floats, or null for the identity
};

// Tables, clears and the launches up to the scan for n checked entries; the counters come back in `res`. With write_thin
// the ordered write of the thin is queued before the counts are read (the map's idle buffer takes it). The device tables
// stay in the block, so that a caller that decides on the counts can still launch a move.
static int run(sf_handle *h, bool thin, int n, const JoinEntry *entries, const sfj_params *params, bool write_thin, std::vector<int> &res,
               const WindowArgs **d_wtab, const JoinArgs **d_jtab, int *max_count_out) {
    HIP_TRY(hipSetDevice(h->device));
    // ---- layout: the two tables; what is cleared to 0 (counters, bids); what is cleared to ~0 (keys); the rest
    SfPlan p;
    const size_t tab_bytes = (size_t)n * (sizeof(WindowArgs) + sizeof(JoinArgs));
    const size_t o_tab = p.take(tab_bytes);
    p.zeros_from_here();
    const size_t o_counts = p.take((size_t)n * SFJ_COUNT_WORDS * sizeof(int));
    std::vector<size_t> o_best((size_t)n), o_keys((size_t)n), o_slot((size_t)n), o_ballots((size_t)n), o_blocks((size_t)n);
    std::vector<int> slots((size_t)n);
    for (int q = 0; q < n; q++) {
        slots[(size_t)q] = sfj_slots_for(entries[q].fill->count);
        if (thin) o_best[(size_t)q] = p.take((size_t)slots[(size_t)q] * 8);
    }
    p.ones_from_here();
    for (int q = 0; q < n; q++) o_keys[(size_t)q] = p.take((size_t)slots[(size_t)q] * 8);
    p.rest_from_here();
    int max_fill = 0, max_count = 0;
    for (int q = 0; q < n; q++) {
        const size_t count = (size_t)entries[q].src->count;
        if (thin) o_slot[(size_t)q] = p.take(count * sizeof(int));
        o_ballots[(size_t)q] = p.take((count + 63) / 64 * 8);
        o_blocks[(size_t)q] = p.take(((count + SFJ_BLOCK - 1) / SFJ_BLOCK + 1) * sizeof(int));
        max_fill = std::max(max_fill, entries[q].fill->count);
        max_count = std::max(max_count, entries[q].src->count);
    }
    if (int e = h->join.grow(h->own, p.off, h->stream)) return e;
    unsigned char *base = h->join.dev;
    // ---- the tables, zeroed: one upload
    WindowArgs *wtab = (WindowArgs *)h->join.zeroed<unsigned char>(tab_bytes);
    JoinArgs *jtab = (JoinArgs *)(wtab + n);
    for (int q = 0; q < n; q++) {
        const JoinEntry &en = entries[q];
        JoinArgs &a = jtab[(size_t)q];
        a.fill = en.fill->buf[0];
        a.src = en.src->buf[0];
        a.dst = thin ? nullptr : en.fill->buf[0] + (size_t)en.fill->count * 12;
        a.fill_count = en.fill->count;
        a.count = en.src->count;
        a.slots = slots[(size_t)q];
        a.log2_slots = sfj_log2_of(a.slots);
        a.inv = 1.0f / params[q].cell;
        a.use_conf = params[q].min_confidence > 0.f;
        a.min_confidence = params[q].min_confidence;
        a.stamp = params[q].stamp;
        for (int k = 0; k < 16; k++) a.T[k] = en.T ? en.T[k] : (k % 5 == 0 ? 1.f : 0.f);
        a.keys = (unsigned long long *)(base + o_keys[(size_t)q]);
        a.best = thin ? (unsigned long long *)(base + o_best[(size_t)q]) : nullptr;
        a.slot_of = thin ? (int *)(base + o_slot[(size_t)q]) : nullptr;
        a.ballots = (unsigned long long *)(base + o_ballots[(size_t)q]);
        a.block_counts = (int *)(base + o_blocks[(size_t)q]);
        a.counts = (int *)(base + o_counts) + (size_t)q * SFJ_COUNT_WORDS;
        WindowArgs &w = wtab[(size_t)q];  // what the scan reads, and for a thin the ordered write
        w.src = a.src;
        w.dst = thin ? en.src->buf[1] : nullptr;
        w.count = a.count;
        w.move_rest = 0;
        w.ballots = a.ballots;
        w.block_counts = a.block_counts;
        w.result = a.counts + SFJ_N_OUT;
    }
    if (int e = h->join.upload(o_tab, wtab, tab_bytes, h->stream)) return e;
    if (int e = p.clear(base, h->stream)) return e;
    const WindowArgs *dw = (const WindowArgs *)(base + o_tab);
    const JoinArgs *dj = (const JoinArgs *)(dw + n);
    // ---- insert, flag, scan (and the thin's write)
    const auto grid = [n](int count) { return dim3((unsigned)((count + SFJ_BLOCK - 1) / SFJ_BLOCK), (unsigned)n); };
    if (max_fill) {
        if (thin)
            hipLaunchKernelGGL(sfj_insert_kernel<true>, grid(max_fill), dim3(SFJ_BLOCK), 0, h->stream, dj);
        else
            hipLaunchKernelGGL(sfj_insert_kernel<false>, grid(max_fill), dim3(SFJ_BLOCK), 0, h->stream, dj);
    }
    if (max_count) {
        if (thin)
            hipLaunchKernelGGL(sfj_thin_flag_kernel, grid(max_count), dim3(SFJ_BLOCK), 0, h->stream, dj);
        else
            hipLaunchKernelGGL(sfj_merge_flag_kernel, grid(max_count), dim3(SFJ_BLOCK), 0, h->stream, dj);
    }
    sfw_launch_scan(h, dw, n);
    if (write_thin && max_count) sfw_launch_write(h, dw, grid(max_count).x, n);
    HIP_TRY(hipGetLastError());
    res.assign((size_t)n * SFJ_COUNT_WORDS, 0);
    if (int e = d2h(h, res.data(), base + o_counts, res.size() * sizeof(int))) return e;
    for (int q = 0; q < n; q++) {
        const int *r = res.data() + (size_t)q * SFJ_COUNT_WORDS;
        if (r[SFJ_ERROR]) return fail(SF_ERR_STATE, "sfj: a probe walk visited every slot of a table");
        if (r[SFJ_N_OUT] < 0 || r[SFJ_N_OUT] > entries[q].src->count) return fail(SF_ERR_DEVICE, "sfj: a count outside the map came back");
    }
    if (d_wtab) *d_wtab = dw;
    if (d_jtab) *d_jtab = dj;
    if (max_count_out) *max_count_out = max_count;
    return SF_OK;
}

static sfj_counts counts_of(const int *r, int n_in) {
    sfj_counts c{};
    c.n_in = n_in;
    c.n_outside = r[SFJ_N_OUTSIDE];
    c.n_voxels = r[SFJ_N_VOXELS];
    c.n_below = r[SFJ_N_BELOW];
    c.n_shared = r[SFJ_N_SHARED];
    c.n_out = r[SFJ_N_OUT];
    return c;
}

extern "C" {

int sfj_version(void) { return SFJ_VERSION; }
size_t sfj_params_bytes(void) { return sizeof(sfj_params); }
size_t sfj_counts_bytes(void) { return sizeof(sfj_counts); }

int sfj_default_params(sfj_params *p) {
    if (!p) return fail(SF_ERR_ARG, "sfj_default_params: null");
    *p = sfj_params{0.02f, 0.0f, -1, 0, {0, 0, 0, 0}};
    return SF_OK;
}

int sfj_check_params(const sfj_params *p) { return check_params(p); }

int sfj_table_slots(int count) {
    if (count < 0 || count > SFJ_MAX_COUNT) return fail(SF_ERR_ARG, "sfj_table_slots: count lies in 0 .. 2^29");
    return sfj_slots_for(count);
}

int sfj_voxel_key(const sfj_params *p, const float pos[3], uint64_t *key) {
    if (!pos || !key) return fail(SF_ERR_ARG, "sfj_voxel_key: null argument");
    if (int e = check_params(p)) return e;
    const float inv = 1.0f / p->cell;
    return sfj_key_of(pos[0], pos[1], pos[2], inv, key) ? 1 : 0;
}

int sfj_hash_slot(uint64_t key, int slots) {
    if (slots < SFJ_MIN_SLOTS || slots > (1 << 30) || (slots & (slots - 1))) return fail(SF_ERR_ARG, "sfj_hash_slot: slots is a power of two in 64 .. 2^30");
    return (int)sfj_first_slot(key, sfj_log2_of(slots));
}

int sfj_thin_maps(sf_handle *h, int n, sf_map *const *maps, const sfj_params *params, sfj_counts *counts_out) {
    if (!h || n < 0 || (n && (!maps || !params || !counts_out))) return fail(SF_ERR_ARG, "sfj_thin_maps: bad argument");
    if (n == 0) return SF_OK;
    if (int e = check_batch("sfj_thin_maps", n)) return e;
    std::vector<JoinEntry> entries((size_t)n);
    bool any_write = false;
    for (int q = 0; q < n; q++) {
        if (int e = check_map("sfj_thin_maps", h, maps[q])) return e;
        if (int e = check_distinct("sfj_thin_maps", maps, q, "the same map twice in one batch")) return e;
        if (int e = check_params(params + q)) return e;
        entries[(size_t)q] = JoinEntry{maps[q], maps[q], nullptr};
        any_write = any_write || !params[q].dry_run;
    }
    std::vector<int> res;
    if (int e = run(h, true, n, entries.data(), params, any_write, res, nullptr, nullptr, nullptr)) return e;
    for (int q = 0; q < n; q++) {  // commit: only after the whole batch has run and its counts are back
        const int *r = res.data() + (size_t)q * SFJ_COUNT_WORDS;
        counts_out[q] = counts_of(r, maps[q]->count);
        if (params[q].dry_run) continue;
        std::swap(maps[q]->buf[0], maps[q]->buf[1]);  // the partitioned buffer becomes the map: its first n_out surfels
        maps[q]->count = r[SFJ_N_OUT];
        indices_moved(maps[q]);
    }
    return SF_OK;
}

int sfj_thin_extract(sf_map *m, const sfj_params *p, float *surfels_out, int max_count, sfj_counts *counts_out) {
    if (!m || !p || !counts_out || max_count < 0 || (!surfels_out && max_count > 0)) return fail(SF_ERR_ARG, "sfj_thin_extract: bad argument");
    sf_handle *h = m->h;
    if (int e = check_map("sfj_thin_extract", h, m)) return e;
    if (int e = check_params(p)) return e;
    const JoinEntry entry{m, m, nullptr};
    std::vector<int> res;
    const WindowArgs *dw = nullptr;
    int max_n = 0;
    if (int e = run(h, true, 1, &entry, p, false, res, &dw, nullptr, &max_n)) return e;
    *counts_out = counts_of(res.data(), m->count);
    const int k = res[SFJ_N_OUT];
    if (k > max_count) return fail(SF_ERR_ARG, "sfj_thin_extract: " + std::to_string(k) + " surfels, room for " + std::to_string(max_count));
    if (k == 0) return SF_OK;
    sfw_launch_write(h, dw, (unsigned)((max_n + SFJ_BLOCK - 1) / SFJ_BLOCK), 1);
    HIP_TRY(hipGetLastError());
    return d2h(h, surfels_out, m->buf[1], (size_t)k * 12 * sizeof(float));
}

int sfj_merge_maps(sf_handle *h, int n, sf_map *const *dst, sf_map *const *src, const float *T, const sfj_params *params, sfj_counts *counts_out) {
    if (!h || n < 0 || (n && (!dst || !src || !params || !counts_out))) return fail(SF_ERR_ARG, "sfj_merge_maps: bad argument");
    if (n == 0) return SF_OK;
    if (int e = check_batch("sfj_merge_maps", n)) return e;
    std::vector<JoinEntry> entries((size_t)n);
    bool any_move = false;
    for (int q = 0; q < n; q++) {
        if (int e = check_map("sfj_merge_maps", h, dst[q])) return e;
        if (int e = check_map("sfj_merge_maps", h, src[q])) return e;
        if (int e = check_distinct("sfj_merge_maps", dst, q, "the same destination twice in one batch")) return e;
        if (int e = check_params(params + q)) return e;
        if (T && !finite_all(T + (size_t)q * 16, 16)) return fail(SF_ERR_ARG, "sfj_merge_maps: NaN or inf in T");
        entries[(size_t)q] = JoinEntry{dst[q], src[q], T ? T + (size_t)q * 16 : nullptr};
        any_move = any_move || !params[q].dry_run;
    }
    for (int q = 0; q < n; q++)
        for (int r = 0; r < n; r++)
            if (src[q] == dst[r]) return fail(SF_ERR_ARG, "sfj_merge_maps: a map is a source and a destination in one batch");
    std::vector<int> res;
    const JoinArgs *dj = nullptr;
    int max_n = 0;
    if (int e = run(h, false, n, entries.data(), params, false, res, nullptr, &dj, &max_n)) return e;
    bool fits = true;
    for (int q = 0; q < n; q++) {
        const int *r = res.data() + (size_t)q * SFJ_COUNT_WORDS;
        counts_out[q] = counts_of(r, src[q]->count);
        if (!params[q].dry_run && (long long)dst[q]->count + r[SFJ_N_OUT] > (long long)dst[q]->capacity) fits = false;
    }
    if (!fits) return fail(SF_ERR_STATE, "sfj_merge_maps: a destination's count + what would be added exceeds its capacity");
    if (!any_move || !max_n) return SF_OK;
    // The move of the entries that are no dry run: their tables go up again with the others' counts set to 0, behind the scan
    // that read them (one stream).
    JoinArgs *jtab = (JoinArgs *)(h->join.host[0].data() + (size_t)n * sizeof(WindowArgs));
    bool changed = false;
    for (int q = 0; q < n; q++)
        if (params[q].dry_run && jtab[(size_t)q].count) {
            jtab[(size_t)q].count = 0;
            changed = true;
        }
    if (changed) HIP_TRY(hipMemcpyAsync((void *)dj, jtab, (size_t)n * sizeof(JoinArgs), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(sfj_merge_move_kernel, dim3((unsigned)((max_n + SFJ_BLOCK - 1) / SFJ_BLOCK), (unsigned)n), dim3(SFJ_BLOCK), 0, h->stream, dj);
    HIP_TRY(hipGetLastError());
    for (int q = 0; q < n; q++)
        if (!params[q].dry_run && res[(size_t)q * SFJ_COUNT_WORDS + SFJ_N_OUT]) {
            dst[q]->count += res[(size_t)q * SFJ_COUNT_WORDS + SFJ_N_OUT];
            indices_moved(dst[q]);
        }
    return SF_OK;
}

}  // extern "C"
