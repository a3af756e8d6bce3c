// sf_hip_carve.hip — libsf_hip.so, the interface of include/sf_carve.h (symbols sfe_*): surfels that later frames saw through are
// taken out of their maps, many maps and many frames per call (kernel: sf_carve.h; the rules host and device share:
// sf_carve_rules.h). A carver owns one call block (sf_call_block.h) under an owner of its own, as a closure builder does. In it
// lie the two map tables of the stable partition (the one the scan reads; the one the ordered write reads, in which a dry run has
// count 0), the carve's map table and the entry table sorted by map, the counts, and per map its ballots, block counts and -- where
// asked for -- vote words; for the host form the uploaded frames come last. One launch votes, the scan of the bounded maps
// (sfw_launch_scan) turns the block counts into offsets and, unless every map is a dry run, their ordered write
// (sfw_launch_write) fills the idle buffers; the counts are read back once, and only a map that lost a surfel swaps its buffers.
// sf_destroy of the handle releases the memory and leaves the carver as an empty shell.
#include "../../include/sf_carve.h"
#include "sf_host.h"
#include "sf_carve.h"

#define SFE_VERSION 1
static_assert(sizeof(sfe_params) == 48, "include/sf_carve.h: sfe_params is 48 bytes");
static_assert(sizeof(sfe_counts) == 32 && sizeof(sfe_counts) == SFE_COUNT_WORDS * sizeof(int), "a map's counts are read back as one record");
static_assert(SFE_CLASS_UNSEEN == SFE_UNSEEN && SFE_CLASS_THROUGH == SFE_THROUGH && SFE_CLASS_SUPPORTED == SFE_SUPPORTED && SFE_CLASS_OCCLUDED == SFE_OCCLUDED,
              "sf_carve_rules.h restates the classes of include/sf_carve.h");
static_assert(offsetof(sfe_params, min_cos) == 12, "the four floats of sfe_params are consecutive");

struct SF_INTERNAL sfe_carver : SfPart {
    SfCallBlock blk;  // host copy 0: the four tables; host copy 1: the counts read back
    void shelled() override { blk.forget(); }
};

static int check_params(const sfe_params *p) {
    if (!p) return fail(SF_ERR_ARG, "sfe: null params");
    if (!finite_all(&p->tol_abs, 4)) return fail(SF_ERR_ARG, "sfe: NaN or inf in sfe_params");
    if (p->tol_abs < 0.f || p->tol_rel < 0.f) return fail(SF_ERR_ARG, "sfe: a negative tolerance");
    if (!(p->z_max > 0.f && p->z_max <= 32.f)) return fail(SF_ERR_ARG, "sfe: z_max lies in (0, 32]");
    if (!(p->min_cos >= 0.f && p->min_cos <= 1.f)) return fail(SF_ERR_ARG, "sfe: min_cos lies in [0, 1]");
    if (p->window < 0 || p->window > SFE_MAX_WINDOW) return fail(SF_ERR_ARG, "sfe: window lies in 0..3");
    const int side = 2 * p->window + 1;
    if (p->min_pixels < 1 || p->min_pixels > side * side) return fail(SF_ERR_ARG, "sfe: min_pixels lies in 1..(2 window + 1)^2");
    if (p->min_votes < 1 || p->min_votes > 65535) return fail(SF_ERR_ARG, "sfe: min_votes lies in 1..65535");
    if (p->max_support < 0 || p->max_support > 65535) return fail(SF_ERR_ARG, "sfe: max_support lies in 0..65535");
    if (p->dry_run != 0 && p->dry_run != 1) return fail(SF_ERR_ARG, "sfe: dry_run is 0 or 1");
    return SF_OK;
}

static SfeRule rule_of(const sfe_params &p) { return SfeRule{p.tol_abs, p.tol_rel, p.z_max, p.min_cos, p.window, p.min_pixels, p.min_votes, p.max_support}; }

// what a surfel reads of a checked view, for a map at `tick`
static SfeView view_of(const sfv_view &v, int tick) {
    SfeView o{};
    invert_pose(v.pose, o.t_inv);
    o.cx = v.cx; o.cy = v.cy; o.fx = v.fx; o.fy = v.fy;
    o.max_depth = v.max_depth;
    o.min_confidence = v.min_confidence;
    o.tick = float(tick);
    o.max_age = float(v.max_age);
    o.use_age = v.max_age >= 0;
    o.rows = v.rows;
    o.cols = v.cols;
    return o;
}

// every check of the refusal list, then: lay out, grow, fill, upload, vote, scan, write, the counts, the votes, commit
static int carve(const char *what, CallForm form, sfe_carver *c, int n_maps, sf_map *const *maps, const sfe_params *params, int n, const int32_t *map_of,
                 const sfv_view *views, const int32_t *streams, const float *const *depth, sfe_counts *counts_out, uint32_t *const *votes_out) {
    const std::string w(what);
    if (int e = check_part(what, c, "carver")) return e;
    sf_handle *h = c->h;
    if (int e = check_batch(w, n_maps, "maps")) return e;
    if (int e = check_batch(w, n)) return e;
    if (n_maps == 0 && n == 0) return SF_OK;
    if (n_maps && (!maps || !params || !counts_out)) return fail(SF_ERR_ARG, w + ": null argument");
    if (n && (!map_of || !views || (form == FORM_STREAMS ? !streams : !depth))) return fail(SF_ERR_ARG, w + ": null argument");
    for (int m = 0; m < n_maps; m++) {
        if (int e = check_map(what, h, maps[m])) return e;
        if (int e = check_distinct(w, maps, m, "the same map twice in one call")) return e;
        if (int e = check_params(params + m)) return e;
    }
    for (int q = 0; q < n; q++) {
        if (map_of[q] < 0 || map_of[q] >= n_maps) return fail(SF_ERR_ARG, w + ": map_of of an entry lies in 0 .. n_maps - 1");
        if (int e = sfv_check_view(views + q)) return e;
        if (form == FORM_STREAMS) {
            if (int e = check_stream(h, streams[q])) return e;  // where sf_get_current refuses, with its code
            if (views[q].rows != h->k.rows || views[q].cols != h->k.cols) return fail(SF_ERR_ARG, w + ": a view of another size than the handle's streams");
        } else {
            if (int e = check_image_size(w, views[q].rows, views[q].cols)) return e;
            if (!depth[q]) return fail(SF_ERR_ARG, w + ": null depth image");
        }
    }
    HIP_TRY(hipSetDevice(h->device));
    // ---- the entries of map m, in the caller's order: order[first[m] .. first[m] + n_entries[m])
    std::vector<int> first((size_t)n_maps + 1, 0), order((size_t)n);
    for (int q = 0; q < n; q++) first[(size_t)map_of[q] + 1]++;
    for (int m = 0; m < n_maps; m++) first[(size_t)m + 1] += first[(size_t)m];
    {
        std::vector<int> next(first.begin(), first.end() - 1);
        for (int q = 0; q < n; q++) order[(size_t)next[(size_t)map_of[q]]++] = q;
    }
    // ---- layout: the four tables (one upload), the counts (zeroed), per map its scratch, the frames of the host form
    SfPlan p;
    const size_t wtab_bytes = (size_t)n_maps * sizeof(WindowArgs), mtab_bytes = (size_t)n_maps * sizeof(CarveMap), etab_bytes = (size_t)n * sizeof(CarveEntry);
    const size_t o_scan = 0, o_write = wtab_bytes, o_mtab = 2 * wtab_bytes, o_etab = 2 * wtab_bytes + mtab_bytes;  // within the tables
    const size_t tab_bytes = o_etab + etab_bytes;
    static_assert(sizeof(WindowArgs) % 8 == 0 && sizeof(CarveMap) % 8 == 0 && sizeof(CarveEntry) % 8 == 0, "the tables follow one another aligned");
    const size_t o_tab = p.take(tab_bytes);
    const size_t counts_bytes = (size_t)n_maps * SFE_COUNT_WORDS * sizeof(int);
    const size_t o_counts = p.take(counts_bytes);
    std::vector<size_t> o_ballots((size_t)n_maps), o_blocks((size_t)n_maps), o_votes((size_t)n_maps), o_frame((size_t)n);
    int max_count = 0, max_write = 0;
    bool any_write = false;
    for (int m = 0; m < n_maps; m++) {
        const size_t count = (size_t)maps[m]->count;
        o_ballots[(size_t)m] = p.take((count + 63) / 64 * 8);
        o_blocks[(size_t)m] = p.take(((count + SFW_BLOCK - 1) / SFW_BLOCK + 1) * sizeof(int));
        if (votes_out && votes_out[m]) o_votes[(size_t)m] = p.take(count * sizeof(unsigned));
        max_count = std::max(max_count, maps[m]->count);
        if (!params[m].dry_run && first[(size_t)m + 1] > first[(size_t)m]) {  // (a map without entries loses nothing)
            any_write = true;
            max_write = std::max(max_write, maps[m]->count);
        }
    }
    if (form == FORM_HOST)
        for (int q = 0; q < n; q++) o_frame[(size_t)q] = p.take((size_t)views[q].rows * views[q].cols * sizeof(float));
    if (int e = c->blk.grow(c->own, p.off, h->stream)) return e;
    unsigned char *base = c->blk.dev;
    // ---- the tables (host copy 0)
    unsigned char *tabs = c->blk.zeroed<unsigned char>(tab_bytes);
    WindowArgs *scan_tab = (WindowArgs *)(tabs + o_scan), *write_tab = (WindowArgs *)(tabs + o_write);
    CarveMap *mtab = (CarveMap *)(tabs + o_mtab);
    CarveEntry *etab = (CarveEntry *)(tabs + o_etab);
    for (int m = 0; m < n_maps; m++) {
        const sf_map *mp = maps[m];
        CarveMap &a = mtab[(size_t)m];
        a.surfels = mp->buf[0];
        a.count = mp->count;
        a.first = first[(size_t)m];
        a.n_entries = first[(size_t)m + 1] - first[(size_t)m];
        a.rule = rule_of(params[m]);
        a.votes = (votes_out && votes_out[m]) ? (unsigned *)(base + o_votes[(size_t)m]) : nullptr;
        a.ballots = (unsigned long long *)(base + o_ballots[(size_t)m]);
        a.block_counts = (int *)(base + o_blocks[(size_t)m]);
        a.counts = (int *)(base + o_counts) + (size_t)m * SFE_COUNT_WORDS;
        WindowArgs &s = scan_tab[(size_t)m];  // what the scan reads ...
        s.src = mp->buf[0];
        s.dst = mp->buf[1];
        s.count = mp->count;
        s.move_rest = 0;
        s.ballots = a.ballots;
        s.block_counts = a.block_counts;
        s.result = a.counts + 6;  // n_out
        write_tab[(size_t)m] = s;  // ... and what the ordered write reads: a map that must stay as it is has nothing to move
        if (params[m].dry_run || a.n_entries == 0) write_tab[(size_t)m].count = 0;
    }
    for (int k = 0; k < n; k++) {
        const int q = order[(size_t)k];
        CarveEntry &en = etab[(size_t)k];
        en.view = view_of(views[q], maps[map_of[q]]->tick);
        if (form == FORM_STREAMS) {
            en.zf = h->k.pyr_new[0] + (size_t)streams[q] * h->k.n_tot;  // what sf_get_current copies out
        } else {
            en.zf = (const float *)(base + o_frame[(size_t)q]);
            HIP_TRY(hipMemcpyAsync(base + o_frame[(size_t)q], depth[q], (size_t)views[q].rows * views[q].cols * sizeof(float), hipMemcpyHostToDevice, h->stream));
        }
    }
    if (int e = c->blk.upload(o_tab, tabs, tab_bytes, h->stream)) return e;
    HIP_TRY(hipMemsetAsync(base + o_counts, 0, counts_bytes, h->stream));
    // ---- vote, scan, write
    const WindowArgs *d_scan = (const WindowArgs *)(base + o_tab + o_scan), *d_write = (const WindowArgs *)(base + o_tab + o_write);
    const auto blocks = [](int count) { return (unsigned)((count + SFW_BLOCK - 1) / SFW_BLOCK); };
    if (max_count)
        hipLaunchKernelGGL(sfe_carve_kernel, dim3(blocks(max_count), (unsigned)n_maps), dim3(SFW_BLOCK), 0, h->stream, (const CarveMap *)(base + o_tab + o_mtab),
                           (const CarveEntry *)(base + o_tab + o_etab));
    sfw_launch_scan(h, d_scan, n_maps);
    if (any_write && max_write) sfw_launch_write(h, d_write, blocks(max_write), n_maps);
    HIP_TRY(hipGetLastError());
    // ---- the counts, once
    int *res = c->blk.resized<int>((size_t)n_maps * SFE_COUNT_WORDS, 1);
    if (int e = d2h(h, res, base + o_counts, counts_bytes)) return e;
    for (int m = 0; m < n_maps; m++) {
        const int *r = res + (size_t)m * SFE_COUNT_WORDS;
        const int count = maps[m]->count;
        if (r[0] != count || r[5] < 0 || r[5] > count || r[6] != count - r[5]) return fail(SF_ERR_DEVICE, w + ": the scan and the counts disagree");
        for (int f = 1; f < 5; f++)
            if (r[f] < 0 || r[f] > count) return fail(SF_ERR_DEVICE, w + ": a count outside the map came back");
    }
    if (votes_out)
        for (int m = 0; m < n_maps; m++)
            if (votes_out[m] && maps[m]->count)
                HIP_TRY(hipMemcpy(votes_out[m], base + o_votes[(size_t)m], (size_t)maps[m]->count * sizeof(unsigned), hipMemcpyDeviceToHost));
    // ---- commit: only after the whole call has run and its counts are back
    for (int m = 0; m < n_maps; m++) {
        const int *r = res + (size_t)m * SFE_COUNT_WORDS;
        sfe_counts o{};
        o.n_in = r[0]; o.n_judged = r[1]; o.n_through = r[2]; o.n_supported = r[3]; o.n_occluded = r[4]; o.n_carved = r[5];
        o.n_out = r[0] - r[5];
        counts_out[m] = o;
        if (params[m].dry_run || r[5] == 0) continue;  // not touched at all
        std::swap(maps[m]->buf[0], maps[m]->buf[1]);  // the partitioned buffer becomes the map: its first n_out surfels
        maps[m]->count = o.n_out;
        indices_moved(maps[m]);
    }
    return SF_OK;
}

extern "C" {

int sfe_version(void) { return SFE_VERSION; }
size_t sfe_params_bytes(void) { return sizeof(sfe_params); }
size_t sfe_counts_bytes(void) { return sizeof(sfe_counts); }

int sfe_default_params(sfe_params *p) {
    if (!p) return fail(SF_ERR_ARG, "sfe_default_params: null");
    *p = sfe_params{0.02f, 0.01f, 8.0f, 0.2f, 1, 5, 2, 0, 0, {0, 0, 0}};
    return SF_OK;
}

int sfe_check_params(const sfe_params *p) { return check_params(p); }

int sfe_observe(const float s[12], int tick, const sfv_view *view, const float *depth, const sfe_params *params, int32_t found[3]) {
    if (!s || !depth || !found) return fail(SF_ERR_ARG, "sfe_observe: null argument");
    if (int e = sfv_check_view(view)) return e;
    if (int e = check_image_size("sfe_observe", view->rows, view->cols)) return e;
    if (int e = check_params(params)) return e;
    const SfeView v = view_of(*view, tick);
    const SfeRule r = rule_of(*params);
    int f[3];
    const int cls = sfe_observe_core(s, &v, depth, &r, f);
    found[0] = f[0]; found[1] = f[1]; found[2] = f[2];
    return cls;
}

int sfe_decide(int v_through, int v_support, const sfe_params *params) {
    if (v_through < 0 || v_through > 65535 || v_support < 0 || v_support > 65535) return fail(SF_ERR_ARG, "sfe_decide: votes lie in 0..65535");
    if (int e = check_params(params)) return e;
    const SfeRule r = rule_of(*params);
    return sfe_decide_core(v_through, v_support, &r) ? 1 : 0;
}

int sfe_carver_create(sf_handle *h, sfe_carver **out) {
    if (!h || !out) return fail(SF_ERR_ARG, "sfe_carver_create: null argument");
    if (int e = check_live_handle("sfe_carver_create", h)) return e;
    sfe_carver *c = new sfe_carver;
    c->h = h;
    h->parts.enter(c);
    *out = c;
    return SF_OK;
}

void sfe_carver_destroy(sfe_carver *c) {
    if (!c) return;
    part_destroy(c);
    delete c;
}

int sfe_carve_streams(sfe_carver *c, int n_maps, sf_map *const *maps, const sfe_params *params, int n, const int32_t *map_of, const sfv_view *views,
                      const int32_t *streams, sfe_counts *counts_out, uint32_t *const *votes_out) {
    return carve("sfe_carve_streams", FORM_STREAMS, c, n_maps, maps, params, n, map_of, views, streams, nullptr, counts_out, votes_out);
}

int sfe_carve_images(sfe_carver *c, int n_maps, sf_map *const *maps, const sfe_params *params, int n, const int32_t *map_of, const sfv_view *views,
                     const float *const *depth, sfe_counts *counts_out, uint32_t *const *votes_out) {
    return carve("sfe_carve_images", FORM_HOST, c, n_maps, maps, params, n, map_of, views, nullptr, depth, counts_out, votes_out);
}

}  // extern "C"
