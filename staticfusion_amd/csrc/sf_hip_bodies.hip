// sf_hip_bodies.hip — libsf_hip.so, the interface of include/sf_bodies.h (symbols sfb_*): the rigid motion of every moving
// region of a batch of frame pairs, by damped point-to-plane steps (kernels: sf_bodies.h; the system: sf_p2p_system.h; the step:
// sf_align_step.h; the state of a region and the step's bookkeeping: sf_p2p_device.h; the world motion: sf_body_world.h). Everything a call needs lies in the call block sf_handle::bodies (sf_call_block.h: layout, growth
// and lifetime): the entry table, the pair table, the region states, the model images, the systems and -- for the host form --
// the uploaded frames and the results. A call only reads its inputs. The number of launches is fixed by the largest
// `iterations` of the call; nothing is read back between them.
#include "../../include/sf_bodies.h"
#include "sf_host.h"
#include "sf_bodies.h"

#define SFB_VERSION 1
static_assert(sizeof(sfb_params) == 32, "include/sf_bodies.h: sfb_params is 32 bytes");
static_assert(sizeof(sfb_motion) == 192, "include/sf_bodies.h: sfb_motion is 192 bytes");
static_assert(sizeof(sfb_camera) == sizeof(sft_camera) && offsetof(sfb_camera, cx) == offsetof(sft_camera, cx) && offsetof(sfb_camera, fy) == offsetof(sft_camera, fy),
              "include/sf_bodies.h: sfb_camera is the camera of include/sf_tracks.h");
static_assert(sizeof(sfb_system) == p2p::WORDS * sizeof(long long) && offsetof(sfb_system, g) == 16 && offsetof(sfb_system, H) == 64 &&
                  offsetof(sfb_system, reserved) == p2p::FIELDS * sizeof(long long),
              "include/sf_bodies.h: sfb_system is the system of sf_p2p_system.h, its summed words first");
static_assert(SFB_OK == p2p::OK && SFB_FEW_PAIRS == p2p::FEW_PAIRS && SFB_DEGENERATE == p2p::DEGENERATE, "include/sf_bodies.h: the status codes of sf_p2p_system.h");
static_assert(SFB_PB % SFB_NT == 0 && SFB_FIELDS <= 64, "sf_bodies.h: one lane per summed word");

static_assert(offsetof(sfb_params, damping) == 12, "the four floats of sfb_params are consecutive");
static int check_params(const sfb_params *p) {
    if (!p) return fail(SF_ERR_ARG, "sfb: null params");
    if (!finite_all(&p->dist_max, 4)) return fail(SF_ERR_ARG, "sfb: NaN or inf in sfb_params");
    if (!(p->dist_max > 0.f && p->dist_max <= 1.f)) return fail(SF_ERR_ARG, "sfb: dist_max lies in (0, 1]");
    if (!(p->z_max > 0.f && p->z_max <= 32.f)) return fail(SF_ERR_ARG, "sfb: z_max lies in (0, 32]");
    if (!(p->normal_dz > 0.f && p->normal_dz <= 32.f)) return fail(SF_ERR_ARG, "sfb: normal_dz lies in (0, 32]");
    if (p->damping < 0.f) return fail(SF_ERR_ARG, "sfb: a negative damping");
    if (p->iterations < 1 || p->iterations > 64) return fail(SF_ERR_ARG, "sfb: iterations lie in 1..64");
    if (p->min_pairs < 6) return fail(SF_ERR_ARG, "sfb: min_pairs is at least 6");
    return SF_OK;
}

// every check of the refusal list, then: plan, grow, upload, the model images, the fixed sequence of linearisations and steps,
// and for the host form the copies back
static int estimate(const char *what, bool device_form, sf_handle *h, int rows, int cols, int n, const void *const *depth0, const void *const *labels0,
                    const void *const *depth1, const void *const *labels1, const sfb_camera *cams0, const sfb_camera *cams1, const int32_t *n_regions,
                    const int32_t *pairs, const sfb_params *params, int max_regions, void *motions, void *systems_out) {
    const std::string w(what);
    if (!h || n < 0) return fail(SF_ERR_ARG, w + ": bad argument");
    if (int e = check_live_handle(w, h)) return e;
    if (n == 0) return SF_OK;
    if (int e = check_batch(w, n)) return e;
    if (!depth0 || !labels0 || !depth1 || !cams0 || !cams1 || !n_regions || !params || !motions) return fail(SF_ERR_ARG, w + ": null argument");
    if (int e = check_image_size(w, rows, cols)) return e;
    if (max_regions < 1 || max_regions > SFB_MAX_REGIONS) return fail(SF_ERR_ARG, w + ": max_regions lies in 1..256");
    const int M = max_regions;
    int max_it = 0;
    for (int q = 0; q < n; q++) {
        if (!depth0[q] || !labels0[q] || !depth1[q]) return fail(SF_ERR_ARG, w + ": null image");
        if (n_regions[q] < 0 || n_regions[q] > M) return fail(SF_ERR_ARG, w + ": n_regions lies in 0..max_regions");
        if (pairs) {
            const bool have_l1 = labels1 && labels1[q];
            for (int t = 0; t < M; t++) {
                const int32_t want = pairs[(size_t)q * M + t];
                if (want < 0) return fail(SF_ERR_ARG, w + ": a negative pair");
                if (want != 0 && t < n_regions[q] && !have_l1) return fail(SF_ERR_ARG, w + ": a pair without the label image of frame 1");
            }
        }
        if (int e = check_camera("sfb", cams0 + q)) return e;
        if (int e = check_camera("sfb", cams1 + q)) return e;
        if (int e = check_params(params + q)) return e;
        max_it = std::max(max_it, params[q].iterations);
    }
    HIP_TRY(hipSetDevice(h->device));
    // ---- layout
    const size_t px = (size_t)rows * cols, slots_total = (size_t)n * M;
    const int sys_slots = systems_out ? max_it + 1 : 1;  // unless the systems are an output, one record per region slot is reused
    const size_t sys_bytes = slots_total * (size_t)sys_slots * sizeof(sfb_system);
    SfPlan p;
    const size_t o_args = p.take((size_t)n * sizeof(BodyArgs));
    const size_t o_pairs = pairs ? p.take(slots_total * 4) : 0;
    const size_t o_state = p.take(slots_total * sizeof(P2pState));
    const size_t o_sys = (device_form && systems_out) ? 0 : p.take(sys_bytes);
    const size_t o_mot = device_form ? 0 : p.take(slots_total * sizeof(sfb_motion));
    const size_t o_model = p.take((size_t)n * px * 2 * sizeof(vfloat4));
    size_t o_up = 0;
    if (!device_form) o_up = p.take((size_t)n * 4 * px * 4);  // depth0, labels0, depth1, labels1 of every entry
    if (int e = h->bodies.grow(h->own, p.off, h->stream)) return e;
    unsigned char *base = h->bodies.dev;
    // ---- the entry table (host copy 0, zeroed) and the pair table (host copy 1)
    BodyArgs *tab = h->bodies.zeroed<BodyArgs>((size_t)n);
    for (int q = 0; q < n; q++) {
        BodyArgs &a = tab[(size_t)q];
        const sfb_params &sp = params[q];
        const void *l1 = labels1 ? labels1[q] : nullptr;
        if (device_form) {
            a.z0 = (const float *)depth0[q];
            a.l0 = (const int *)labels0[q];
            a.z1 = (const float *)depth1[q];
            a.l1 = (const int *)l1;
        } else {
            unsigned char *up = base + o_up + (size_t)q * 4 * px * 4;
            HIP_TRY(hipMemcpyAsync(up, depth0[q], px * 4, hipMemcpyHostToDevice, h->stream));
            HIP_TRY(hipMemcpyAsync(up + px * 4, labels0[q], px * 4, hipMemcpyHostToDevice, h->stream));
            HIP_TRY(hipMemcpyAsync(up + 2 * px * 4, depth1[q], px * 4, hipMemcpyHostToDevice, h->stream));
            if (l1) HIP_TRY(hipMemcpyAsync(up + 3 * px * 4, l1, px * 4, hipMemcpyHostToDevice, h->stream));
            a.z0 = (const float *)up;
            a.l0 = (const int *)(up + px * 4);
            a.z1 = (const float *)(up + 2 * px * 4);
            a.l1 = l1 ? (const int *)(up + 3 * px * 4) : nullptr;
        }
        a.pairs = pairs ? (const int *)(base + o_pairs) + (size_t)q * M : nullptr;
        a.model = (vfloat4 *)(base + o_model) + (size_t)q * px * 2;
        const sfb_camera &c0 = cams0[q], &c1 = cams1[q];
        a.cx0 = c0.cx; a.cy0 = c0.cy; a.fx0 = c0.fx; a.fy0 = c0.fy;
        a.cx1 = c1.cx; a.cy1 = c1.cy; a.fx1 = c1.fx; a.fy1 = c1.fy;
        std::memcpy(a.pose0, c0.pose, sizeof(a.pose0));
        std::memcpy(a.pose1, c1.pose, sizeof(a.pose1));
        if (int e = sft_relative(c0.pose, c1.pose, a.D0)) return e;  // (both were checked: it does not fail)
        a.dist_max = sp.dist_max; a.z_max = sp.z_max; a.normal_dz = sp.normal_dz; a.damping = sp.damping;
        a.iterations = sp.iterations; a.min_pairs = sp.min_pairs; a.K = n_regions[q];
    }
    const BodyArgs *d_args = (const BodyArgs *)(base + o_args);
    P2pState *d_state = (P2pState *)(base + o_state);
    long long *d_sys = (device_form && systems_out) ? (long long *)systems_out : (long long *)(base + o_sys);
    sfb_motion *d_mot = device_form ? (sfb_motion *)motions : (sfb_motion *)(base + o_mot);
    if (int e = h->bodies.upload(o_args, tab, (size_t)n * sizeof(BodyArgs), h->stream)) return e;
    if (pairs) {
        int32_t *ptab = h->bodies.resized<int32_t>(slots_total, 1);
        std::memcpy(ptab, pairs, slots_total * 4);
        if (int e = h->bodies.upload(o_pairs, ptab, slots_total * 4, h->stream)) return e;
    }
    HIP_TRY(hipMemsetAsync(d_sys, 0, sys_bytes, h->stream));
    HIP_TRY(hipMemsetAsync(d_mot, 0, slots_total * sizeof(sfb_motion), h->stream));  // records K .. M - 1 stay zeros
    // ---- the model images, then the fixed sequence
    const unsigned un = (unsigned)n;
    hipLaunchKernelGGL(sfb_model_kernel, dim3((unsigned)((px + SFB_NT - 1) / SFB_NT), un), dim3(SFB_NT), 0, h->stream, d_args, rows, cols, M, d_state);
    const int keep = systems_out ? 1 : 0;
    for (int it = 0; it <= max_it; it++) {
        const int slot = keep ? it : 0;
        hipLaunchKernelGGL(sfb_linearise_kernel, dim3((unsigned)((px + SFB_PB - 1) / SFB_PB), un), dim3(SFB_NT), 0, h->stream, d_args, rows, cols, M,
                           (const P2pState *)d_state, d_sys, sys_slots, slot, it);
        hipLaunchKernelGGL(sfb_step_kernel, dim3((unsigned)((slots_total + 63) / 64)), dim3(64), 0, h->stream, d_args, (int)slots_total, M, d_state, d_sys, sys_slots,
                           slot, keep, d_mot, it);
    }
    HIP_TRY(hipGetLastError());
    if (device_form) return SF_OK;
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(motions, d_mot, slots_total * sizeof(sfb_motion), hipMemcpyDeviceToHost));
    if (systems_out) HIP_TRY(hipMemcpy(systems_out, d_sys, sys_bytes, hipMemcpyDeviceToHost));
    return SF_OK;
}

extern "C" {

int sfb_version(void) { return SFB_VERSION; }
size_t sfb_params_bytes(void) { return sizeof(sfb_params); }
size_t sfb_motion_bytes(void) { return sizeof(sfb_motion); }
size_t sfb_camera_bytes(void) { return sizeof(sfb_camera); }
size_t sfb_system_bytes(void) { return sizeof(sfb_system); }

int sfb_default_params(sfb_params *p) {
    if (!p) return fail(SF_ERR_ARG, "sfb_default_params: null");
    *p = sfb_params{0.10f, 8.0f, 0.05f, 0.0f, 10, 64, {0, 0}};
    return SF_OK;
}

int sfb_check_params(const sfb_params *p) { return check_params(p); }

int sfb_world_motion(const float pose0[16], const float pose1[16], const double D[12], float w_out[16]) {
    if (!pose0 || !pose1 || !D || !w_out) return fail(SF_ERR_ARG, "sfb_world_motion: null argument");
    bool finite = finite_all(pose0, 16) && finite_all(pose1, 16);
    for (int k = 0; k < 12; k++) finite = finite && std::isfinite(D[k]);
    if (!finite) return fail(SF_ERR_ARG, "sfb_world_motion: NaN or inf in an input");
    float w[16];
    sfb_world_core(pose0, pose1, D, w);
    std::memcpy(w_out, w, sizeof(w));
    return SF_OK;
}

int sfb_estimate_images(sf_handle *h, int rows, int cols, int n, const float *const *depth0, const int32_t *const *labels0, const float *const *depth1,
                        const int32_t *const *labels1, const sfb_camera *cams0, const sfb_camera *cams1, const int32_t *n_regions, const int32_t *pairs,
                        const sfb_params *params, int max_regions, sfb_motion *motions_out, sfb_system *systems_out) {
    return estimate("sfb_estimate_images", false, h, rows, cols, n, (const void *const *)depth0, (const void *const *)labels0, (const void *const *)depth1,
                    (const void *const *)labels1, cams0, cams1, n_regions, pairs, params, max_regions, motions_out, systems_out);
}

int sfb_estimate_images_device(sf_handle *h, int rows, int cols, int n, const void *const *depth0, const void *const *labels0, const void *const *depth1,
                               const void *const *labels1, const sfb_camera *cams0, const sfb_camera *cams1, const int32_t *n_regions, const int32_t *pairs,
                               const sfb_params *params, int max_regions, void *motions_out, void *systems_out) {
    return estimate("sfb_estimate_images_device", true, h, rows, cols, n, depth0, labels0, depth1, labels1, cams0, cams1, n_regions, pairs, params, max_regions,
                    motions_out, systems_out);
}

}  // extern "C"
