// sf_hip_score.hip — libsf_hip.so, the interface of include/sf_score.h (symbols sfs_*): frame-to-map agreement counts of many
// (map, view, frame) entries per call (kernel: sf_score.h). The maps are drawn by the drawing stage of the views
// (sfv_plan / sfv_draw_keys of sf_hip_view.hip) into the call block sf_handle::score (sf_call_block.h: layout, growth and
// lifetime); behind the drawing layout lie the score table, the result records and -- for the host-pointer calls -- the
// uploaded frames and the class images. A score call only reads its maps and streams.
#include "../../include/sf_score.h"
#include "sf_host.h"
#include "sf_score.h"

#define SFS_VERSION 1
static_assert(sizeof(sfs_params) == 32, "include/sf_score.h: sfs_params is 32 bytes");
static_assert(sizeof(sfs_score) == 96, "include/sf_score.h: sfs_score is 96 bytes");
static_assert(sizeof(sfs_score) == 12 * sizeof(long long) && SFS_FIELDS == 10, "sfs_score_kernel adds the first ten int64 fields");

static_assert(offsetof(sfs_params, b_min) == 12, "the four floats of sfs_params are consecutive");
static int check_params(const sfs_params *p) {
    if (!p) return fail(SF_ERR_ARG, "sfs: null params");
    if (!finite_all(&p->tol_abs, 4)) return fail(SF_ERR_ARG, "sfs: NaN or inf in sfs_params");
    if (p->tol_abs < 0.f || p->tol_rel < 0.f) return fail(SF_ERR_ARG, "sfs: a negative tolerance");
    if (!(p->max_residual > 0.f && p->max_residual <= 32.f)) return fail(SF_ERR_ARG, "sfs: max_residual lies in (0, 32]");
    if ((p->use_grey != 0 && p->use_grey != 1) || (p->use_b != 0 && p->use_b != 1)) return fail(SF_ERR_ARG, "sfs: use_grey and use_b are 0 or 1");
    return SF_OK;
}

// every check of the refusal list, then: plan, grow, upload, draw, score, and for the host forms the copies back
static int score(const char *what, CallForm form, sf_handle *h, int n, sf_map *const *maps, const sfv_view *views, const int32_t *streams,
                 const void *const *depth, const void *const *grey, const void *const *b, const sfs_params *params, void *scores,
                 void *const *class_out) {
    const std::string w(what);
    if (!h || n < 0) return fail(SF_ERR_ARG, w + ": bad argument");
    if (n == 0) return SF_OK;
    if (!maps || !views || !params || !scores || (form == FORM_STREAMS ? !streams : !depth)) return fail(SF_ERR_ARG, w + ": null argument");
    if (int e = check_batch(w, n)) return e;
    std::vector<ViewJob> jobs((size_t)n);
    for (int q = 0; q < n; q++) {
        const sf_map *m = maps[q];
        if (int e = check_map(what, h, m)) return e;
        if (int e = sfv_check_view(views + q)) return e;
        if (int e = check_params(params + q)) return e;
        if (form == FORM_STREAMS) {
            if (int e = check_stream(h, streams[q])) return e;  // where sf_get_current / sf_get_b_image refuse, with their code
            if (views[q].rows != h->k.rows || views[q].cols != h->k.cols) return fail(SF_ERR_ARG, w + ": a view of another size than the handle's streams");
        } else {
            if (!depth[q]) return fail(SF_ERR_ARG, w + ": null depth image");
            if (params[q].use_grey && !(grey && grey[q])) return fail(SF_ERR_ARG, w + ": use_grey without a grey image");
            if (params[q].use_b && !(b && b[q])) return fail(SF_ERR_ARG, w + ": use_b without a b image");
        }
        jobs[(size_t)q] = ViewJob{m->buf[0], m->count, m->tick};
    }
    HIP_TRY(hipSetDevice(h->device));
    // ---- layout: the drawing stage, then what the score kernel reads and writes
    ViewPlan p;
    sfv_plan(p, n, jobs.data(), views, 0);
    const size_t o_stab = p.take((size_t)n * sizeof(ScoreArgs));
    const size_t o_rec = form == FORM_DEVICE ? 0 : p.take((size_t)n * sizeof(sfs_score));
    std::vector<size_t> o_depth((size_t)n), o_grey((size_t)n), o_b((size_t)n), o_cls((size_t)n);
    size_t max_px = 0;
    for (int q = 0; q < n; q++) {
        const size_t px = (size_t)views[q].rows * views[q].cols;
        max_px = std::max(max_px, px);
        if (form == FORM_HOST) {
            o_depth[(size_t)q] = p.take(px * 4);
            if (params[q].use_grey) o_grey[(size_t)q] = p.take(px * 4);
            if (params[q].use_b) o_b[(size_t)q] = p.take(px * 4);
        }
        if (form != FORM_DEVICE && class_out && class_out[q]) o_cls[(size_t)q] = p.take(px);
    }
    if (int e = h->score.grow(h->own, p.off, h->stream)) return e;
    unsigned char *base = h->score.dev;
    // ---- the score table (host copy 1; the view table is copy 0)
    ScoreArgs *stab = h->score.resized<ScoreArgs>((size_t)n, 1);
    long long *d_rec = form == FORM_DEVICE ? (long long *)scores : (long long *)(base + o_rec);
    for (int q = 0; q < n; q++) {
        ScoreArgs &s = stab[(size_t)q];
        const sfs_params &sp = params[q];
        const size_t px = (size_t)views[q].rows * views[q].cols;
        if (form == FORM_STREAMS) {
            const size_t st = (size_t)streams[q];
            s.depth = h->k.pyr_new[0] + st * h->k.n_tot;  // what sf_get_current and sf_get_b_image copy out
            s.grey = h->k.pyr_new[1] + st * h->k.n_tot;
            s.b = h->k.b_img + st * h->k.n0;
        } else if (form == FORM_HOST) {
            s.depth = (const float *)(base + o_depth[(size_t)q]);
            s.grey = sp.use_grey ? (const float *)(base + o_grey[(size_t)q]) : nullptr;
            s.b = sp.use_b ? (const float *)(base + o_b[(size_t)q]) : nullptr;
            HIP_TRY(hipMemcpyAsync(base + o_depth[(size_t)q], depth[q], px * 4, hipMemcpyHostToDevice, h->stream));
            if (sp.use_grey) HIP_TRY(hipMemcpyAsync(base + o_grey[(size_t)q], grey[q], px * 4, hipMemcpyHostToDevice, h->stream));
            if (sp.use_b) HIP_TRY(hipMemcpyAsync(base + o_b[(size_t)q], b[q], px * 4, hipMemcpyHostToDevice, h->stream));
        } else {
            s.depth = (const float *)depth[q];
            s.grey = sp.use_grey ? (const float *)grey[q] : nullptr;
            s.b = sp.use_b ? (const float *)b[q] : nullptr;
        }
        s.tol_abs = sp.tol_abs; s.tol_rel = sp.tol_rel; s.max_residual = sp.max_residual; s.b_min = sp.b_min;
        s.use_grey = sp.use_grey; s.use_b = sp.use_b;
        s.score = d_rec + (size_t)q * (sizeof(sfs_score) / sizeof(long long));
        if (form == FORM_DEVICE) s.cls = class_out ? (uint8_t *)class_out[q] : nullptr;
        else s.cls = (class_out && class_out[q]) ? base + o_cls[(size_t)q] : nullptr;
    }
    if (int e = h->score.upload(o_stab, stab, (size_t)n * sizeof(ScoreArgs), h->stream)) return e;
    HIP_TRY(hipMemsetAsync(d_rec, 0, (size_t)n * sizeof(sfs_score), h->stream));
    // ---- draw the keys, then score
    if (int e = sfv_draw_keys(h, p, jobs.data(), views, nullptr, h->score, nullptr, 0)) return e;
    const unsigned per_block = SFS_NT * SFS_PER_THREAD;
    hipLaunchKernelGGL(sfs_score_kernel, dim3((unsigned)((max_px + per_block - 1) / per_block), (unsigned)n), dim3(SFS_NT), 0, h->stream,
                       (const ViewArgs *)(base + p.o_tab), (const ScoreArgs *)(base + o_stab));
    HIP_TRY(hipGetLastError());
    if (form == FORM_DEVICE) return SF_OK;
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(scores, d_rec, (size_t)n * sizeof(sfs_score), hipMemcpyDeviceToHost));
    for (int q = 0; q < n; q++)
        if (class_out && class_out[q])
            HIP_TRY(hipMemcpy(class_out[q], base + o_cls[(size_t)q], (size_t)views[q].rows * views[q].cols, hipMemcpyDeviceToHost));
    return SF_OK;
}

extern "C" {

int sfs_version(void) { return SFS_VERSION; }
size_t sfs_params_bytes(void) { return sizeof(sfs_params); }
size_t sfs_score_bytes(void) { return sizeof(sfs_score); }

int sfs_default_params(sfs_params *p) {
    if (!p) return fail(SF_ERR_ARG, "sfs_default_params: null");
    *p = sfs_params{0.02f, 0.01f, 8.0f, 0.5f, 1, 1, {0, 0}};
    return SF_OK;
}

int sfs_check_params(const sfs_params *p) { return check_params(p); }

int sfs_score_streams(sf_handle *h, int n, sf_map *const *maps, const sfv_view *views, const int32_t *streams, const sfs_params *params,
                      sfs_score *scores, uint8_t *const *class_out) {
    return score("sfs_score_streams", FORM_STREAMS, h, n, maps, views, streams, nullptr, nullptr, nullptr, params, scores, (void *const *)class_out);
}

int sfs_score_images(sf_handle *h, int n, sf_map *const *maps, const sfv_view *views, const float *const *depth, const float *const *grey,
                     const float *const *b, const sfs_params *params, sfs_score *scores, uint8_t *const *class_out) {
    return score("sfs_score_images", FORM_HOST, h, n, maps, views, nullptr, (const void *const *)depth, (const void *const *)grey, (const void *const *)b,
                 params, scores, (void *const *)class_out);
}

int sfs_score_images_device(sf_handle *h, int n, sf_map *const *maps, const sfv_view *views, const void *const *depth, const void *const *grey,
                            const void *const *b, const sfs_params *params, void *scores, void *const *class_out) {
    return score("sfs_score_images_device", FORM_DEVICE, h, n, maps, views, nullptr, depth, grey, b, params, scores, class_out);
}

}  // extern "C"
