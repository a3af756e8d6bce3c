// sf_hip_align.hip — libsf_hip.so, the interface of include/sf_align.h (symbols sfa_*): damped point-to-plane refinement of
// many (map, candidate pose, frame) entries per call (kernels: sf_align.h; the system: sf_p2p_system.h; the step: sf_align_step.h;
// the state of an entry and the step's bookkeeping: sf_p2p_device.h). The maps are drawn by
// the drawing stage of the views (sfv_plan / sfv_draw_keys of sf_hip_view.hip) into the call block sf_handle::align
// (sf_call_block.h: layout, growth and lifetime); behind the drawing layout lie the entry table with the entries' states, the
// model images, the systems, the result records and -- for the host-pointer calls -- the uploaded frames. A refine call only
// reads its maps and streams. The number of launches is fixed by the largest `iterations` of the call; nothing is read back
// between them.
#include "../../include/sf_align.h"
#include "sf_host.h"
#include "sf_align.h"

#define SFA_VERSION 1
static_assert(sizeof(sfa_params) == 32, "include/sf_align.h: sfa_params is 32 bytes");
static_assert(sizeof(sfa_result) == 128, "include/sf_align.h: sfa_result is 128 bytes");
static_assert(sizeof(sfa_system) == p2p::WORDS * sizeof(long long) && offsetof(sfa_system, reserved) == p2p::FIELDS * sizeof(long long),
              "include/sf_align.h: sfa_system is the system of sf_p2p_system.h, its summed words first");
static_assert(SFA_OK == p2p::OK && SFA_FEW_PAIRS == p2p::FEW_PAIRS && SFA_DEGENERATE == p2p::DEGENERATE, "include/sf_align.h: the status codes of sf_p2p_system.h");

static_assert(offsetof(sfa_params, damping) == 12, "the four floats of sfa_params are consecutive");
static int check_params(const sfa_params *p) {
    if (!p) return fail(SF_ERR_ARG, "sfa: null params");
    if (!finite_all(&p->dist_max, 4)) return fail(SF_ERR_ARG, "sfa: NaN or inf in sfa_params");
    if (!(p->dist_max > 0.f && p->dist_max <= 1.f)) return fail(SF_ERR_ARG, "sfa: dist_max lies in (0, 1]");
    if (!(p->z_max > 0.f && p->z_max <= 32.f)) return fail(SF_ERR_ARG, "sfa: z_max lies in (0, 32]");
    if (p->damping < 0.f) return fail(SF_ERR_ARG, "sfa: a negative damping");
    if (p->iterations < 1 || p->iterations > 64) return fail(SF_ERR_ARG, "sfa: iterations lie in 1..64");
    if (p->stride < 1 || p->stride > 16) return fail(SF_ERR_ARG, "sfa: stride lies in 1..16");
    if (p->min_pairs < 6) return fail(SF_ERR_ARG, "sfa: min_pairs is at least 6");
    if (p->use_b != 0 && p->use_b != 1) return fail(SF_ERR_ARG, "sfa: use_b is 0 or 1");
    return SF_OK;
}

// every check of the refusal list, then: plan, grow, upload, draw, model images, the fixed sequence of linearisations and
// steps, and for the host forms the copies back
static int refine(const char *what, CallForm form, sf_handle *h, int n, sf_map *const *maps, const sfv_view *views, const int32_t *streams,
                  const void *const *depth, const void *const *b, const sfa_params *params, void *results, void *systems_out) {
    const std::string w(what);
    if (!h || n < 0) return fail(SF_ERR_ARG, w + ": bad argument");
    if (n == 0) return SF_OK;
    if (!maps || !views || !params || !results || (form == FORM_STREAMS ? !streams : !depth)) return fail(SF_ERR_ARG, w + ": null argument");
    if (int e = check_batch(w, n)) return e;
    std::vector<ViewJob> jobs((size_t)n);
    int max_it = 0;
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
            if (params[q].use_b && !(b && b[q])) return fail(SF_ERR_ARG, w + ": use_b without a b image");
        }
        jobs[(size_t)q] = ViewJob{m->buf[0], m->count, m->tick};
        max_it = std::max(max_it, params[q].iterations);
    }
    HIP_TRY(hipSetDevice(h->device));
    // ---- layout: the drawing stage, then what the three kernels read and write
    const size_t sys_bytes = (size_t)n * (size_t)(max_it + 1) * sizeof(sfa_system);
    ViewPlan p;
    sfv_plan(p, n, jobs.data(), views, 0);
    const size_t tab_bytes = (size_t)n * (sizeof(AlignArgs) + sizeof(P2pState));  // the table, then the states: one upload
    const size_t o_atab = p.take(tab_bytes);
    const size_t o_state = o_atab + (size_t)n * sizeof(AlignArgs);
    const size_t o_res = form == FORM_DEVICE ? 0 : p.take((size_t)n * sizeof(sfa_result));
    const size_t o_sys = (form == FORM_DEVICE && systems_out) ? 0 : p.take(sys_bytes);
    std::vector<size_t> o_model((size_t)n), o_depth((size_t)n), o_b((size_t)n);
    size_t max_px = 0, max_sub = 0;
    for (int q = 0; q < n; q++) {
        const size_t px = (size_t)views[q].rows * views[q].cols;
        const size_t st = (size_t)params[q].stride;
        max_px = std::max(max_px, px);
        max_sub = std::max(max_sub, (((size_t)views[q].rows + st - 1) / st) * (((size_t)views[q].cols + st - 1) / st));
        o_model[(size_t)q] = p.take(px * 2 * sizeof(vfloat4));
        if (form == FORM_HOST) {
            o_depth[(size_t)q] = p.take(px * 4);
            if (params[q].use_b) o_b[(size_t)q] = p.take(px * 4);
        }
    }
    if (int e = h->align.grow(h->own, p.off, h->stream)) return e;
    unsigned char *base = h->align.dev;
    // ---- the entry table and the states (host copy 1, zeroed: a state starts from zeros; the view table is copy 0)
    AlignArgs *atab = (AlignArgs *)h->align.zeroed<unsigned char>(tab_bytes, 1);
    P2pState *states = (P2pState *)(atab + n);
    sfa_result *d_res = form == FORM_DEVICE ? (sfa_result *)results : (sfa_result *)(base + o_res);
    long long *d_sys = (form == FORM_DEVICE && systems_out) ? (long long *)systems_out : (long long *)(base + o_sys);
    for (int q = 0; q < n; q++) {
        AlignArgs &s = atab[(size_t)q];
        const sfa_params &sp = params[q];
        const size_t px = (size_t)views[q].rows * views[q].cols;
        if (form == FORM_STREAMS) {
            const size_t st = (size_t)streams[q];
            s.depth = h->k.pyr_new[0] + st * h->k.n_tot;  // what sf_get_current and sf_get_b_image copy out
            s.b = h->k.b_img + st * h->k.n0;
        } else if (form == FORM_HOST) {
            s.depth = (const float *)(base + o_depth[(size_t)q]);
            s.b = sp.use_b ? (const float *)(base + o_b[(size_t)q]) : nullptr;
            HIP_TRY(hipMemcpyAsync(base + o_depth[(size_t)q], depth[q], px * 4, hipMemcpyHostToDevice, h->stream));
            if (sp.use_b) HIP_TRY(hipMemcpyAsync(base + o_b[(size_t)q], b[q], px * 4, hipMemcpyHostToDevice, h->stream));
        } else {
            s.depth = (const float *)depth[q];
            s.b = sp.use_b ? (const float *)b[q] : nullptr;
        }
        s.dist_max = sp.dist_max; s.z_max = sp.z_max; s.b_min = sp.b_min; s.damping = sp.damping;
        s.iterations = sp.iterations; s.stride = sp.stride; s.min_pairs = sp.min_pairs; s.use_b = sp.use_b;
        for (int k = 0; k < 16; k++) s.t0[k] = views[q].pose[k];
        s.model = (vfloat4 *)(base + o_model[(size_t)q]);
        s.systems = d_sys + (size_t)q * (size_t)(max_it + 1) * p2p::WORDS;
        s.state = (P2pState *)(base + o_state) + q;
        s.result = d_res + q;
        states[(size_t)q].D[0] = states[(size_t)q].D[5] = states[(size_t)q].D[10] = 1.0;  // D0 = I
    }
    if (int e = h->align.upload(o_atab, atab, tab_bytes, h->stream)) return e;
    HIP_TRY(hipMemsetAsync(d_sys, 0, sys_bytes, h->stream));
    // ---- draw the keys, resolve the model images, then the fixed sequence
    if (int e = sfv_draw_keys(h, p, jobs.data(), views, nullptr, h->align, nullptr, 0)) return e;
    const ViewArgs *d_vtab = (const ViewArgs *)(base + p.o_tab);
    const AlignArgs *d_atab = (const AlignArgs *)(base + o_atab);
    hipLaunchKernelGGL(sfa_model_kernel, dim3((unsigned)((max_px + 255) / 256), (unsigned)n), dim3(256), 0, h->stream, d_vtab, d_atab);
    const unsigned per_block = SFA_NT * SFA_PER_THREAD;
    for (int it = 0; it <= max_it; it++) {
        hipLaunchKernelGGL(sfa_linearise_kernel, dim3((unsigned)((max_sub + per_block - 1) / per_block), (unsigned)n), dim3(SFA_NT), 0, h->stream, d_vtab,
                           d_atab, it);
        hipLaunchKernelGGL(sfa_step_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, h->stream, d_atab, n, it);
    }
    HIP_TRY(hipGetLastError());
    if (form == FORM_DEVICE) return SF_OK;
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(results, d_res, (size_t)n * sizeof(sfa_result), hipMemcpyDeviceToHost));
    if (systems_out) HIP_TRY(hipMemcpy(systems_out, d_sys, sys_bytes, hipMemcpyDeviceToHost));
    return SF_OK;
}

extern "C" {

int sfa_version(void) { return SFA_VERSION; }
size_t sfa_params_bytes(void) { return sizeof(sfa_params); }
size_t sfa_result_bytes(void) { return sizeof(sfa_result); }
size_t sfa_system_bytes(void) { return sizeof(sfa_system); }

int sfa_default_params(sfa_params *p) {
    if (!p) return fail(SF_ERR_ARG, "sfa_default_params: null");
    *p = sfa_params{0.15f, 8.0f, 0.5f, 0.0f, 10, 1, 64, 1};
    return SF_OK;
}

int sfa_check_params(const sfa_params *p) { return check_params(p); }

int sfa_step(const sfa_system *s, float damping, const double D_in[12], double D_out[12]) {
    if (!s || !D_in || !D_out) return fail(SF_ERR_ARG, "sfa_step: null argument");
    return sfa_step_core((const int64_t *)s, damping, D_in, D_out);
}

int sfa_refine_streams(sf_handle *h, int n, sf_map *const *maps, const sfv_view *views, const int32_t *streams, const sfa_params *params,
                       sfa_result *results, sfa_system *systems_out) {
    return refine("sfa_refine_streams", FORM_STREAMS, h, n, maps, views, streams, nullptr, nullptr, params, results, systems_out);
}

int sfa_refine_images(sf_handle *h, int n, sf_map *const *maps, const sfv_view *views, const float *const *depth, const float *const *b,
                      const sfa_params *params, sfa_result *results, sfa_system *systems_out) {
    return refine("sfa_refine_images", FORM_HOST, h, n, maps, views, nullptr, (const void *const *)depth, (const void *const *)b, params, results,
                  systems_out);
}

int sfa_refine_images_device(sf_handle *h, int n, sf_map *const *maps, const sfv_view *views, const void *const *depth, const void *const *b,
                             const sfa_params *params, void *results, void *systems_out) {
    return refine("sfa_refine_images_device", FORM_DEVICE, h, n, maps, views, nullptr, depth, b, params, results, systems_out);
}

}  // extern "C"
