// sf_hip_body_maps.hip — libsf_hip.so, the interface of include/sf_body_maps.h (symbols sfp_*): every moving region fused into
// a surfel map of its own, many per call (kernels: sf_body_maps.h; the per-surfel rules: sf_body_map_rules.h; key, rank and
// hash: sf_join_key.h). The two entry tables, the counters, the voxel tables with their bids, the candidates' slots, the merge
// table, the ballots, the block counts and -- for the host form -- the uploaded frames of a call lie in the call block
// sf_handle::body_maps (sf_call_block.h: layout, growth and lifetime); the scan is that of the bounded maps (sfw_launch_scan).
// One host synchronisation reads the counts; it lies before the two passes that change a map, because the capacity test needs
// them.
#include "../../include/sf_body_maps.h"
#include "sf_host.h"
#include "sf_body_maps.h"

#define SFP_VERSION 1
static_assert(sizeof(sfp_params) == 32, "include/sf_body_maps.h: sfp_params is 32 bytes");
static_assert(sizeof(sfp_counts) == 32, "include/sf_body_maps.h: sfp_counts is 32 bytes");
static_assert(sizeof(sfp_counts) == SFP_COUNT_WORDS * sizeof(int), "an entry's counters are read back as one record");
static_assert(sizeof(sfp_camera) == sizeof(sft_camera) && offsetof(sfp_camera, pose) == offsetof(sft_camera, pose) && offsetof(sfp_camera, cx) == offsetof(sft_camera, cx) &&
                  offsetof(sfp_camera, cy) == offsetof(sft_camera, cy) && offsetof(sfp_camera, fx) == offsetof(sft_camera, fx) &&
                  offsetof(sfp_camera, fy) == offsetof(sft_camera, fy) && sizeof(sfp_camera) == 80,
              "include/sf_body_maps.h: sfp_camera is the camera of include/sf_tracks.h");

static int check_params(const sfp_params *p) {
    if (!p) return fail(SF_ERR_ARG, "sfp: null params");
    if (!finite_all(&p->cell, 7)) return fail(SF_ERR_ARG, "sfp: NaN or inf in sfp_params");
    if (!(p->cell > 0.f)) return fail(SF_ERR_ARG, "sfp: cell is finite and > 0");
    if (!std::isfinite(1.0f / p->cell)) return fail(SF_ERR_ARG, "sfp: 1 / cell is not finite");
    if (!(p->z_max > 0.f && p->z_max <= 32.f)) return fail(SF_ERR_ARG, "sfp: z_max lies in (0, 32]");
    if (!(p->normal_dz > 0.f && p->normal_dz <= 32.f)) return fail(SF_ERR_ARG, "sfp: normal_dz lies in (0, 32]");
    if (!(p->min_dot >= -1.f && p->min_dot <= 1.f)) return fail(SF_ERR_ARG, "sfp: min_dot lies in [-1, 1]");
    if (!(p->conf_new >= 0.f && p->conf_new <= 1.f)) return fail(SF_ERR_ARG, "sfp: conf_new lies in [0, 1]");
    if (!(p->gain > 0.f && p->gain <= 1.f)) return fail(SF_ERR_ARG, "sfp: gain lies in (0, 1]");
    if (!(p->max_weight >= 1.f)) return fail(SF_ERR_ARG, "sfp: max_weight is at least 1");
    return SF_OK;
}
static_assert(offsetof(sfp_params, max_weight) == 24, "the seven floats of sfp_params are consecutive");

// h is a live handle, the n maps are its own and distinct, W is finite
static int check_maps(const std::string &w, sf_handle *h, int n, sf_map *const *maps, const float *W) {
    for (int q = 0; q < n; q++) {
        if (int e = check_map(w.c_str(), h, maps[q])) return e;
        if (int e = check_distinct(w, maps, q, "the same map twice in one call")) return e;
        if (W && !finite_all(W + (size_t)q * 16, 16)) return fail(SF_ERR_ARG, w + ": NaN or inf in W");
    }
    return SF_OK;
}

static void set_motion(BodyMapArgs &a, const float *W, int q) {
    for (int k = 0; k < 16; k++) a.W[k] = W ? W[(size_t)q * 16 + k] : (k % 5 == 0 ? 1.f : 0.f);
}

// every check of the refusal list, then: plan, grow, upload, insert, pixels, flag, scan, the counts, the capacity, the commit
static int fuse(const char *what, bool device_form, sf_handle *h, int rows, int cols, int n, const void *const *depth, const void *const *labels,
                const void *const *colour, const sfp_camera *cams, const int32_t *region_labels, sf_map *const *maps, const float *W, const sfp_params *params,
                sfp_counts *counts_out) {
    const std::string w(what);
    if (!h || n < 0) return fail(SF_ERR_ARG, w + ": bad argument");
    if (int e = check_live_handle(w, h)) return e;
    if (n == 0) return SF_OK;
    if (int e = check_batch(w, n)) return e;
    if (!depth || !labels || !cams || !region_labels || !maps || !params || !counts_out) return fail(SF_ERR_ARG, w + ": null argument");
    if (int e = check_image_size(w, rows, cols)) return e;
    for (int q = 0; q < n; q++) {
        if (!depth[q] || !labels[q]) return fail(SF_ERR_ARG, w + ": null image");
        if (region_labels[q] < 1) return fail(SF_ERR_ARG, w + ": a region label below 1");
        if (int e = check_camera("sfp", cams + q)) return e;
        if (int e = check_params(params + q)) return e;
    }
    if (int e = check_maps(w, h, n, maps, W)) return e;
    HIP_TRY(hipSetDevice(h->device));
    // ---- layout: the two tables; what is cleared to 0 (counters, bids of the surfels, ballots, block counts); what is cleared
    // to ~0 (keys, bids of the pixels, the merge table); the rest
    const size_t px = (size_t)rows * cols;
    const size_t interior = (size_t)std::max(rows - 2, 0) * (size_t)std::max(cols - 2, 0);
    const size_t n_blocks = (px + SFP_BLOCK - 1) / SFP_BLOCK;
    SfPlan p;
    const size_t tab_bytes = (size_t)n * (sizeof(WindowArgs) + sizeof(BodyMapArgs));
    const size_t o_tab = p.take(tab_bytes);
    p.zeros_from_here();
    const size_t o_counts = p.take((size_t)n * SFP_COUNT_WORDS * sizeof(int));
    std::vector<size_t> o_best((size_t)n), o_ballots((size_t)n), o_blocks((size_t)n), o_keys((size_t)n), o_bid((size_t)n), o_merge((size_t)n), o_cand((size_t)n);
    std::vector<int> slots((size_t)n);
    int max_count = 0;
    for (int q = 0; q < n; q++) {
        const size_t elements = (size_t)maps[q]->count + interior;
        if (elements > (size_t)SFJ_MAX_COUNT) return fail(SF_ERR_ARG, w + ": a map too large for a voxel table");
        slots[(size_t)q] = sfj_slots_for((int)elements);
        o_best[(size_t)q] = p.take((size_t)slots[(size_t)q] * 8);
        o_ballots[(size_t)q] = p.take((px + 63) / 64 * 8);
        o_blocks[(size_t)q] = p.take((n_blocks + 1) * sizeof(int));
        max_count = std::max(max_count, maps[q]->count);
    }
    p.ones_from_here();
    for (int q = 0; q < n; q++) {
        o_keys[(size_t)q] = p.take((size_t)slots[(size_t)q] * 8);
        o_bid[(size_t)q] = p.take((size_t)slots[(size_t)q] * 4);
        o_merge[(size_t)q] = p.take((size_t)maps[q]->count * sizeof(int));
    }
    p.rest_from_here();
    for (int q = 0; q < n; q++) o_cand[(size_t)q] = p.take(px * sizeof(int));
    const size_t frame_bytes = (px * 4 + 255) / 256 * 256 * 2 + (px * 3 + 255) / 256 * 256;  // depth, labels, colour of an entry
    const size_t o_up = device_form ? 0 : p.take((size_t)n * frame_bytes);
    if (int e = h->body_maps.grow(h->own, p.off, h->stream)) return e;
    unsigned char *base = h->body_maps.dev;
    // ---- the tables, zeroed: one upload
    WindowArgs *wtab = (WindowArgs *)h->body_maps.zeroed<unsigned char>(tab_bytes);
    BodyMapArgs *atab = (BodyMapArgs *)(wtab + n);
    for (int q = 0; q < n; q++) {
        BodyMapArgs &a = atab[(size_t)q];
        const sfp_params &sp = params[q];
        const void *rgb = colour ? colour[q] : nullptr;
        if (device_form) {
            a.z = (const float *)depth[q];
            a.lab = (const int *)labels[q];
            a.rgb = (const uint8_t *)rgb;
        } else {
            unsigned char *up = base + o_up + (size_t)q * frame_bytes;
            const size_t plane = (px * 4 + 255) / 256 * 256;
            HIP_TRY(hipMemcpyAsync(up, depth[q], px * 4, hipMemcpyHostToDevice, h->stream));
            HIP_TRY(hipMemcpyAsync(up + plane, labels[q], px * 4, hipMemcpyHostToDevice, h->stream));
            if (rgb) HIP_TRY(hipMemcpyAsync(up + 2 * plane, rgb, px * 3, hipMemcpyHostToDevice, h->stream));
            a.z = (const float *)up;
            a.lab = (const int *)(up + plane);
            a.rgb = rgb ? (const uint8_t *)(up + 2 * plane) : nullptr;
        }
        a.map = maps[q]->buf[0];
        a.count = maps[q]->count;
        a.t = region_labels[q];
        a.slots = slots[(size_t)q];
        a.log2_slots = sfj_log2_of(a.slots);
        a.cx = cams[q].cx; a.cy = cams[q].cy; a.fx = cams[q].fx; a.fy = cams[q].fy;
        std::memcpy(a.pose, cams[q].pose, sizeof(a.pose));
        set_motion(a, W, q);
        a.inv = 1.0f / sp.cell;
        a.z_max = sp.z_max; a.normal_dz = sp.normal_dz; a.min_dot = sp.min_dot; a.conf_new = sp.conf_new; a.gain = sp.gain; a.max_weight = sp.max_weight;
        a.time = (float)maps[q]->tick;
        a.keys = (unsigned long long *)(base + o_keys[(size_t)q]);
        a.best = (unsigned long long *)(base + o_best[(size_t)q]);
        a.bid = (unsigned *)(base + o_bid[(size_t)q]);
        a.cand_slot = (int *)(base + o_cand[(size_t)q]);
        a.merge_of = (int *)(base + o_merge[(size_t)q]);
        a.ballots = (unsigned long long *)(base + o_ballots[(size_t)q]);
        a.block_counts = (int *)(base + o_blocks[(size_t)q]);
        a.counts = (int *)(base + o_counts) + (size_t)q * SFP_COUNT_WORDS;
        WindowArgs &sw = wtab[(size_t)q];  // what the scan reads: the block counts over pixels
        sw.count = (int)px;
        sw.ballots = a.ballots;
        sw.block_counts = a.block_counts;
        sw.result = a.counts + SFP_N_ADDED;
    }
    if (int e = h->body_maps.upload(o_tab, wtab, tab_bytes, h->stream)) return e;
    if (int e = p.clear(base, h->stream)) return e;
    const WindowArgs *dw = (const WindowArgs *)(base + o_tab);
    const BodyMapArgs *da = (const BodyMapArgs *)(dw + n);
    // ---- insert, pixels, flag, scan
    const dim3 pixel_grid((unsigned)n_blocks, (unsigned)n), surfel_grid((unsigned)((max_count + SFP_BLOCK - 1) / SFP_BLOCK), (unsigned)n);
    if (max_count) hipLaunchKernelGGL(sfp_insert_kernel, surfel_grid, dim3(SFP_BLOCK), 0, h->stream, da);
    hipLaunchKernelGGL(sfp_pixel_kernel, pixel_grid, dim3(SFP_BLOCK), 0, h->stream, da, rows, cols);
    hipLaunchKernelGGL(sfp_flag_kernel, pixel_grid, dim3(SFP_BLOCK), 0, h->stream, da, rows, cols);
    sfw_launch_scan(h, dw, n);
    HIP_TRY(hipGetLastError());
    std::vector<int> res((size_t)n * SFP_COUNT_WORDS, 0);
    if (int e = d2h(h, res.data(), base + o_counts, res.size() * sizeof(int))) return e;
    for (int q = 0; q < n; q++) {
        const int *r = res.data() + (size_t)q * SFP_COUNT_WORDS;
        if (r[SFP_ERROR]) return fail(SF_ERR_STATE, w + ": a probe walk visited every slot of a table");
        if (r[SFP_N_ADDED] < 0 || (size_t)r[SFP_N_ADDED] > interior) return fail(SF_ERR_DEVICE, w + ": a count outside the frame came back");
    }
    bool fits = true;
    for (int q = 0; q < n; q++) {
        const int *r = res.data() + (size_t)q * SFP_COUNT_WORDS;
        sfp_counts c{};
        c.n_pixels = r[SFP_N_PIXELS];
        c.n_candidates = r[SFP_N_CANDIDATES];
        c.n_voxels = r[SFP_N_VOXELS];
        c.n_merged = r[SFP_N_MERGED];
        c.n_added = r[SFP_N_ADDED];
        c.n_conflict = r[SFP_N_CONFLICT];
        c.n_out = maps[q]->count + r[SFP_N_ADDED];
        counts_out[q] = c;
        if ((long long)maps[q]->count + r[SFP_N_ADDED] > (long long)maps[q]->capacity) fits = false;
    }
    if (!fits) return fail(SF_ERR_STATE, w + ": a map's count + what would be added exceeds its capacity");
    // ---- commit: move and merge in place, then the ordered append
    if (max_count) hipLaunchKernelGGL(sfp_move_kernel<true>, surfel_grid, dim3(SFP_BLOCK), 0, h->stream, da, rows, cols);
    hipLaunchKernelGGL(sfp_append_kernel, pixel_grid, dim3(SFP_BLOCK), 0, h->stream, da, rows, cols);
    HIP_TRY(hipGetLastError());
    for (int q = 0; q < n; q++) {
        sf_map *m = maps[q];
        m->count += res[(size_t)q * SFP_COUNT_WORDS + SFP_N_ADDED];
        m->tick += 1;
        std::memcpy(m->pose, cams[q].pose, sizeof(m->pose));
        indices_moved(m);
    }
    return SF_OK;
}

extern "C" {

int sfp_version(void) { return SFP_VERSION; }
size_t sfp_params_bytes(void) { return sizeof(sfp_params); }
size_t sfp_counts_bytes(void) { return sizeof(sfp_counts); }
size_t sfp_camera_bytes(void) { return sizeof(sfp_camera); }

int sfp_default_params(sfp_params *p) {
    if (!p) return fail(SF_ERR_ARG, "sfp_default_params: null");
    *p = sfp_params{0.01f, 8.0f, 0.05f, 0.8f, 0.1f, 0.25f, 32.0f, 0};
    return SF_OK;
}

int sfp_check_params(const sfp_params *p) { return check_params(p); }

int sfp_pixel_surfel(const float depths[5], int v, int u, const sfp_camera *cam, const uint8_t *colour, const sfp_params *p, float time, float out[12]) {
    if (!depths || !cam || !out) return fail(SF_ERR_ARG, "sfp_pixel_surfel: null argument");
    if (int e = check_params(p)) return e;
    if (int e = check_camera("sfp", cam)) return e;
    const int r = colour ? colour[0] : 128, g = colour ? colour[1] : 128, b = colour ? colour[2] : 128;
    float s[12];
    if (!sfp_pixel_surfel_core(depths, v, u, cam->pose, cam->cx, cam->cy, cam->fx, cam->fy, r, g, b, p->z_max, p->normal_dz, p->conf_new, time, s)) return 0;
    std::memcpy(out, s, sizeof(s));
    return 1;
}

int sfp_merge_surfel(const sfp_params *p, const float s[12], const float pixel[12], float time, float out[12]) {
    if (!s || !pixel || !out) return fail(SF_ERR_ARG, "sfp_merge_surfel: null argument");
    if (int e = check_params(p)) return e;
    sfp_merge_core(s, pixel, p->gain, p->max_weight, time, out);
    return SF_OK;
}

int sfp_move_maps(sf_handle *h, int n, sf_map *const *maps, const float *W) {
    const std::string w("sfp_move_maps");
    if (!h || n < 0) return fail(SF_ERR_ARG, w + ": bad argument");
    if (int e = check_live_handle(w, h)) return e;
    if (n == 0) return SF_OK;
    if (int e = check_batch(w, n)) return e;
    if (!maps) return fail(SF_ERR_ARG, w + ": null argument");
    if (int e = check_maps(w, h, n, maps, W)) return e;
    HIP_TRY(hipSetDevice(h->device));
    const size_t tab_bytes = (size_t)n * sizeof(BodyMapArgs);
    if (int e = h->body_maps.grow(h->own, tab_bytes, h->stream)) return e;
    BodyMapArgs *atab = h->body_maps.zeroed<BodyMapArgs>((size_t)n);
    int max_count = 0;
    for (int q = 0; q < n; q++) {
        atab[(size_t)q].map = maps[q]->buf[0];
        atab[(size_t)q].count = maps[q]->count;
        set_motion(atab[(size_t)q], W, q);
        max_count = std::max(max_count, maps[q]->count);
    }
    if (int e = h->body_maps.upload(0, atab, tab_bytes, h->stream)) return e;
    if (max_count)
        hipLaunchKernelGGL(sfp_move_kernel<false>, dim3((unsigned)((max_count + SFP_BLOCK - 1) / SFP_BLOCK), (unsigned)n), dim3(SFP_BLOCK), 0, h->stream,
                           (const BodyMapArgs *)h->body_maps.dev, 0, 0);
    HIP_TRY(hipGetLastError());
    for (int q = 0; q < n; q++) indices_moved(maps[q]);
    return SF_OK;
}

int sfp_fuse_images(sf_handle *h, int rows, int cols, int n, const float *const *depth, const int32_t *const *labels, const uint8_t *const *colour,
                    const sfp_camera *cams, const int32_t *region_labels, sf_map *const *maps, const float *W, const sfp_params *params,
                    sfp_counts *counts_out) {
    return fuse("sfp_fuse_images", false, h, rows, cols, n, (const void *const *)depth, (const void *const *)labels, (const void *const *)colour, cams, region_labels,
                maps, W, params, counts_out);
}

int sfp_fuse_images_device(sf_handle *h, int rows, int cols, int n, const void *const *depth, const void *const *labels, const void *const *colour,
                           const sfp_camera *cams, const int32_t *region_labels, sf_map *const *maps, const float *W, const sfp_params *params,
                           sfp_counts *counts_out) {
    return fuse("sfp_fuse_images_device", true, h, rows, cols, n, depth, labels, colour, cams, region_labels, maps, W, params, counts_out);
}

}  // extern "C"
