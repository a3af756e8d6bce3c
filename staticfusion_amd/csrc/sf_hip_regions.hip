// sf_hip_regions.hip — libsf_hip.so, the interface of include/sf_regions.h (symbols sfr_*): connected components of the moving
// pixels of many frames per call, numbered, with one integer record per region (kernels: sf_regions.h). A call's scratch --
// the entry table, the provisional label image and the count image of every entry, the block counts of the numbering and,
// for the host forms, the uploaded frames, the records and the label images -- is the call block sf_handle::regions
// (sf_call_block.h: layout, growth and lifetime). A call only reads its streams.
#include "../../include/sf_regions.h"
#include "sf_host.h"
#include "sf_regions.h"

#define SFR_VERSION 1
static_assert(sizeof(sfr_params) == 32, "include/sf_regions.h: sfr_params is 32 bytes");
static_assert(sizeof(sfr_region) == 64, "include/sf_regions.h: sfr_region is 64 bytes");
static_assert(sizeof(sfr_summary) == 32, "include/sf_regions.h: sfr_summary is 32 bytes");
static_assert(SFR_NB == 4 * SFR_NT && SFR_TV == 64 && (SFR_TV * SFR_TU) % SFR_NT == 0 && SFR_RUN == 8, "sf_regions.h: the lanes' shares");

static_assert(offsetof(sfr_params, dz_rel) == 12, "the four floats of sfr_params are consecutive");
static int check_params(const sfr_params *p) {
    if (!p) return fail(SF_ERR_ARG, "sfr: null params");
    if (!finite_all(&p->z_max, 4)) return fail(SF_ERR_ARG, "sfr: NaN or inf in sfr_params");
    if (!(p->z_max > 0.f && p->z_max <= 32.f)) return fail(SF_ERR_ARG, "sfr: z_max lies in (0, 32]");
    if (p->dz_abs < 0.f || p->dz_rel < 0.f) return fail(SF_ERR_ARG, "sfr: a negative dz_abs or dz_rel");
    if (p->connectivity != 4 && p->connectivity != 8) return fail(SF_ERR_ARG, "sfr: connectivity is 4 or 8");
    if (p->min_pixels < 1) return fail(SF_ERR_ARG, "sfr: min_pixels < 1");
    if (p->use_b != 0 && p->use_b != 1) return fail(SF_ERR_ARG, "sfr: use_b is 0 or 1");
    return SF_OK;
}

// every check of the refusal list, then: grow, upload, the seven launches, and for the host forms the copies back
static int label(const char *what, CallForm form, sf_handle *h, int rows, int cols, int n, const int32_t *streams, const void *const *depth,
                 const void *const *b, const sfr_params *params, int max_regions, void *summaries, void *regions, void *const *labels) {
    const std::string w(what);
    if (!h || n < 0) return fail(SF_ERR_ARG, w + ": bad argument");
    if (n == 0) return SF_OK;
    if (!params || !summaries || (form == FORM_STREAMS ? !streams : !depth)) return fail(SF_ERR_ARG, w + ": null argument");
    if (int e = check_batch(w, n)) return e;
    if (max_regions < 0 || max_regions > 65535) return fail(SF_ERR_ARG, w + ": max_regions lies in 0..65535");
    if (max_regions > 0 && !regions) return fail(SF_ERR_ARG, w + ": null regions_out with max_regions > 0");
    if (form == FORM_STREAMS) {
        rows = h->k.rows;
        cols = h->k.cols;
    }
    if (int e = check_image_size(w, rows, cols)) return e;
    for (int q = 0; q < n; q++) {
        if (int e = check_params(params + q)) return e;
        if (form == FORM_STREAMS) {
            if (int e = check_stream(h, streams[q])) return e;  // where sf_get_current / sf_get_b_image refuse, with their code
        } else {
            if (!depth[q]) return fail(SF_ERR_ARG, w + ": null depth image");
            if (params[q].use_b && !(b && b[q])) return fail(SF_ERR_ARG, w + ": use_b without a b image");
        }
    }
    HIP_TRY(hipSetDevice(h->device));
    // ---- layout
    const RgGeom g = rg_geometry(rows, cols);
    const size_t px = (size_t)g.px;
    SfPlan p;
    const size_t o_args = p.take((size_t)n * sizeof(RgArgs));
    const size_t o_prov = p.take((size_t)n * g.pxs * 4);
    const size_t o_cnt = p.take((size_t)n * g.pxs * 4);
    const size_t o_blocks = p.take((size_t)n * g.blocks * 4);
    size_t o_sum = 0, o_reg = 0;
    std::vector<size_t> o_depth, o_b, o_lab;
    if (form != FORM_DEVICE) {
        o_sum = p.take((size_t)n * sizeof(sfr_summary));
        o_reg = p.take((size_t)n * max_regions * sizeof(sfr_region));
        o_depth.assign((size_t)n, 0);
        o_b.assign((size_t)n, 0);
        o_lab.assign((size_t)n, 0);
        for (int q = 0; q < n; q++) {
            if (form == FORM_HOST) {
                o_depth[(size_t)q] = p.take(px * 4);
                if (params[q].use_b) o_b[(size_t)q] = p.take(px * 4);
            }
            if (labels && labels[q]) o_lab[(size_t)q] = p.take(px * 4);
        }
    }
    if (int e = h->regions.grow(h->own, p.off, h->stream)) return e;
    unsigned char *base = h->regions.dev;
    // ---- the entry table
    RgArgs *tab = h->regions.resized<RgArgs>((size_t)n);
    for (int q = 0; q < n; q++) {
        RgArgs &a = tab[(size_t)q];
        const sfr_params &sp = params[q];
        if (form == FORM_STREAMS) {
            const size_t st = (size_t)streams[q];
            a.depth = h->k.pyr_new[0] + st * h->k.n_tot;  // what sf_get_current and sf_get_b_image copy out
            a.b = sp.use_b ? h->k.b_img + st * h->k.n0 : nullptr;
        } else if (form == FORM_HOST) {
            a.depth = (const float *)(base + o_depth[(size_t)q]);
            a.b = sp.use_b ? (const float *)(base + o_b[(size_t)q]) : nullptr;
            HIP_TRY(hipMemcpyAsync(base + o_depth[(size_t)q], depth[q], px * 4, hipMemcpyHostToDevice, h->stream));
            if (sp.use_b) HIP_TRY(hipMemcpyAsync(base + o_b[(size_t)q], b[q], px * 4, hipMemcpyHostToDevice, h->stream));
        } else {
            a.depth = (const float *)depth[q];
            a.b = sp.use_b ? (const float *)b[q] : nullptr;
        }
        if (form == FORM_DEVICE) a.labels = labels ? (int *)labels[q] : nullptr;
        else a.labels = (labels && labels[q]) ? (int *)(base + o_lab[(size_t)q]) : nullptr;
        a.z_max = sp.z_max; a.b_max = sp.b_max; a.dz_abs = sp.dz_abs; a.dz_rel = sp.dz_rel;
        a.conn8 = sp.connectivity == 8; a.min_pixels = sp.min_pixels; a.use_b = sp.use_b; a.pad = 0;
    }
    const RgArgs *d_args = (const RgArgs *)(base + o_args);
    int *d_prov = (int *)(base + o_prov), *d_cnt = (int *)(base + o_cnt), *d_blocks = (int *)(base + o_blocks);
    sfr_summary *d_sum = form == FORM_DEVICE ? (sfr_summary *)summaries : (sfr_summary *)(base + o_sum);
    sfr_region *d_reg = form == FORM_DEVICE ? (sfr_region *)regions : (sfr_region *)(base + o_reg);
    if (int e = h->regions.upload(o_args, tab, (size_t)n * sizeof(RgArgs), h->stream)) return e;
    HIP_TRY(hipMemsetAsync(d_sum, 0, (size_t)n * sizeof(sfr_summary), h->stream));
    // ---- the seven launches: every grid-wide order is a launch boundary
    const unsigned un = (unsigned)n;
    const unsigned run_blocks = (unsigned)((px + (size_t)SFR_NT * SFR_RUN - 1) / ((size_t)SFR_NT * SFR_RUN));
    hipLaunchKernelGGL(sfr_tile_kernel, dim3((unsigned)(g.tiles_v * g.tiles_u), un), dim3(SFR_NT), 0, h->stream, d_args, g, d_prov, d_cnt);
    if (g.items > 0)
        hipLaunchKernelGGL(sfr_border_kernel, dim3((unsigned)((g.items + SFR_NT - 1) / SFR_NT), un), dim3(SFR_NT), 0, h->stream, d_args, g, d_prov);
    hipLaunchKernelGGL(sfr_flatten_kernel, dim3(run_blocks, un), dim3(SFR_NT), 0, h->stream, g, d_prov, d_cnt);
    hipLaunchKernelGGL(sfr_count_kernel, dim3((unsigned)g.blocks, un), dim3(SFR_NT), 0, h->stream, d_args, g, (const int *)d_prov, (const int *)d_cnt, d_blocks,
                       d_sum);
    hipLaunchKernelGGL(sfr_scan_kernel, dim3(un), dim3(SFR_SCAN_NT), 0, h->stream, g, d_blocks, max_regions, d_sum, d_reg);
    hipLaunchKernelGGL(sfr_number_kernel, dim3((unsigned)g.blocks, un), dim3(SFR_NT), 0, h->stream, d_args, g, (const int *)d_prov, d_cnt,
                       (const int *)d_blocks, max_regions, d_reg);
    hipLaunchKernelGGL(sfr_final_kernel, dim3(run_blocks, un), dim3(SFR_NT), 0, h->stream, d_args, g, (const int *)d_prov, (const int *)d_cnt, max_regions,
                       d_reg);
    HIP_TRY(hipGetLastError());
    if (form == FORM_DEVICE) return SF_OK;
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(summaries, d_sum, (size_t)n * sizeof(sfr_summary), hipMemcpyDeviceToHost));
    if (max_regions > 0) HIP_TRY(hipMemcpy(regions, d_reg, (size_t)n * max_regions * sizeof(sfr_region), hipMemcpyDeviceToHost));
    for (int q = 0; q < n; q++)
        if (labels && labels[q]) HIP_TRY(hipMemcpy(labels[q], base + o_lab[(size_t)q], px * 4, hipMemcpyDeviceToHost));
    return SF_OK;
}

extern "C" {

int sfr_version(void) { return SFR_VERSION; }
size_t sfr_params_bytes(void) { return sizeof(sfr_params); }
size_t sfr_region_bytes(void) { return sizeof(sfr_region); }
size_t sfr_summary_bytes(void) { return sizeof(sfr_summary); }

int sfr_default_params(sfr_params *p) {
    if (!p) return fail(SF_ERR_ARG, "sfr_default_params: null");
    *p = sfr_params{8.0f, 0.5f, 0.05f, 0.02f, 8, 16, 1, 0};
    return SF_OK;
}

int sfr_check_params(const sfr_params *p) { return check_params(p); }

int sfr_label_streams(sf_handle *h, int n, const int32_t *streams, const sfr_params *params, int max_regions, sfr_summary *summaries_out,
                      sfr_region *regions_out, int32_t *const *labels_out) {
    return label("sfr_label_streams", FORM_STREAMS, h, 0, 0, n, streams, nullptr, nullptr, params, max_regions, summaries_out, regions_out,
                 (void *const *)labels_out);
}

int sfr_label_images(sf_handle *h, int rows, int cols, int n, const float *const *depth, const float *const *b, const sfr_params *params,
                     int max_regions, sfr_summary *summaries_out, sfr_region *regions_out, int32_t *const *labels_out) {
    return label("sfr_label_images", FORM_HOST, h, rows, cols, n, nullptr, (const void *const *)depth, (const void *const *)b, params, max_regions,
                 summaries_out, regions_out, (void *const *)labels_out);
}

int sfr_label_images_device(sf_handle *h, int rows, int cols, int n, const void *const *depth, const void *const *b, const sfr_params *params,
                            int max_regions, void *summaries_out, void *regions_out, void *const *labels_out) {
    return label("sfr_label_images_device", FORM_DEVICE, h, rows, cols, n, nullptr, depth, b, params, max_regions, summaries_out, regions_out, labels_out);
}

}  // extern "C"
