// sf_hip_tracks.hip — libsf_hip.so, the interface of include/sf_tracks.h (symbols sft_*): the moving regions of
// include/sf_regions.h followed from frame to frame (kernels: sf_tracks.h; the assignment: sf_track_assign.h). A tracker's
// state -- per slot the head, the camera, the rows and the previous frame's clipped labels and depth -- is one block, and
// its scratch -- the entry table, the records, summaries and label images of the labelling, the overlap tables and, for the
// host forms, the uploaded frames and the outputs of a call -- a call block (sft_tracker::scratch; sf_call_block.h: layout,
// growth and lifetime), both under the tracker's own owner, as a keyframe database has one (sf_parts.h).
// The labelling is sfr_label_images_device as it is: its own scratch is the handle's regions block. What the host keeps per
// slot is what it handed in itself: whether the slot holds a previous frame, and that frame's camera.
#include "../../include/sf_tracks.h"
#include "sf_host.h"
#include "sf_tracks.h"

#define SFT_VERSION 1
static_assert(sizeof(sft_camera) == 80, "include/sf_tracks.h: sft_camera is 80 bytes");
static_assert(sizeof(sft_params) == 32, "include/sf_tracks.h: sft_params is 32 bytes");
static_assert(sizeof(sft_track) == 136, "include/sf_tracks.h: sft_track is 136 bytes");
static_assert(sizeof(sft_summary) == 32, "include/sf_tracks.h: sft_summary is 32 bytes");
static_assert(sizeof(sft_info) == 32 && sizeof(sft_slot) == 16, "include/sf_tracks.h: sft_info is 32 bytes, sft_slot 16");
static_assert(sizeof(TkSlotHead) == 64 && SFT_MAX_TRACKS == SFT_NT && SFT_PB % SFT_NT == 0, "sf_tracks.h: one lane per row of the assignment");

struct SF_INTERNAL sft_tracker : SfPart {
    int rows = 0, cols = 0, n_slots = 0, max_tracks = 0;
    TkLayout lay{};
    unsigned char *state = nullptr;    // n_slots * lay.stride bytes (zero-filled: every slot is fresh)
    SfCallBlock scratch;               // what one call uploads, computes and reads back (host copy 0: the entry table of an
                                       // update, host copy 1: the slots of a reset)
    std::vector<unsigned char> has_prev;  // per slot: it holds a previous frame
    std::vector<sft_camera> cams;         // per slot: that frame's camera
    void shelled() override {
        state = nullptr;
        scratch.forget();
    }
};

static int check_track_params(const sft_params *p) {
    if (!p) return fail(SF_ERR_ARG, "sft: null params");
    if (p->min_overlap < 1) return fail(SF_ERR_ARG, "sft: min_overlap < 1");
    if (p->min_share < 0 || p->min_share > 1024) return fail(SF_ERR_ARG, "sft: min_share lies in 0..1024");
    if (p->use_depth_gate != 0 && p->use_depth_gate != 1) return fail(SF_ERR_ARG, "sft: use_depth_gate is 0 or 1");
    if (!finite_all(&p->dz_abs, 2)) return fail(SF_ERR_ARG, "sft: NaN or inf in sft_params");
    if (p->dz_abs < 0.f || p->dz_rel < 0.f) return fail(SF_ERR_ARG, "sft: a negative dz_abs or dz_rel");
    return SF_OK;
}

// D of the header: fp64, one rounding per entry; bit-equal poses give the exact identity
static int relative(const float *p0, const float *p1, float *D) {
    if (!finite_all(p0, 16) || !finite_all(p1, 16)) return fail(SF_ERR_ARG, "sft_relative: NaN or inf in a pose");
    for (int i = 0; i < 16; i++) D[i] = (i % 5 == 0) ? 1.f : 0.f;
    if (std::memcmp(p0, p1, 16 * sizeof(float)) == 0) return SF_OK;
    double d[3];
    for (int r = 0; r < 3; r++) d[r] = (double)p0[12 + r] - (double)p1[12 + r];
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) {
            const double a = (double)p1[0 + 4 * i] * (double)p0[0 + 4 * j];
            const double b = (double)p1[1 + 4 * i] * (double)p0[1 + 4 * j];
            const double c = (double)p1[2 + 4 * i] * (double)p0[2 + 4 * j];
            const double ab = a + b;
            D[i + 4 * j] = (float)(ab + c);
        }
        const double a = (double)p1[0 + 4 * i] * d[0];
        const double b = (double)p1[1 + 4 * i] * d[1];
        const double c = (double)p1[2 + 4 * i] * d[2];
        const double ab = a + b;
        D[i + 12] = (float)(ab + c);
    }
    return SF_OK;
}

static int check_tracker(const char *what, const sft_tracker *t) { return check_part(what, t, "tracker"); }

static TkLayout slot_layout(int rows, int cols, int max_tracks) {
    SfPlan p;
    TkLayout l;
    p.take(sizeof(TkSlotHead));
    l.o_cam = p.take(sizeof(sft_camera));
    l.o_id = p.take((size_t)max_tracks * 4);
    l.o_birth = p.take((size_t)max_tracks * 4);
    l.o_count = p.take((size_t)max_tracks * 4);
    l.o_labels = p.take((size_t)rows * cols * 4);
    l.o_depth = p.take((size_t)rows * cols * 4);
    l.stride = p.off;
    return l;
}

// every check of the refusal list, then: grow, upload, the labelling, the three launches, and for the host forms the copies back
static int update(const char *what, CallForm form, sft_tracker *t, int rows, int cols, int n, const int32_t *slots, const int32_t *streams,
                  const void *const *depth, const void *const *b, const sft_camera *cameras, const sfr_params *rparams, const sft_params *tparams, void *summaries,
                  void *tracks, void *const *ids) {
    const std::string w(what);
    if (int e = check_tracker(what, t)) return e;
    if (int e = check_batch(w, n)) return e;
    if (n == 0) return SF_OK;
    if (!slots || !cameras || !rparams || !tparams || !summaries || !tracks || (form == FORM_STREAMS ? !streams : !depth))
        return fail(SF_ERR_ARG, w + ": null argument");
    sf_handle *h = t->h;
    if (form == FORM_STREAMS) {
        if (t->rows != h->k.rows || t->cols != h->k.cols) return fail(SF_ERR_ARG, w + ": a tracker of another size than the handle's streams");
        rows = t->rows;
        cols = t->cols;
    } else if (rows != t->rows || cols != t->cols) {
        return fail(SF_ERR_ARG, w + ": rows and cols are not the tracker's");
    }
    std::vector<unsigned char> seen((size_t)t->n_slots, 0);
    for (int q = 0; q < n; q++) {
        if (slots[q] < 0 || slots[q] >= t->n_slots) return fail(SF_ERR_ARG, w + ": slot out of range");
        if (seen[(size_t)slots[q]]) return fail(SF_ERR_ARG, w + ": the same slot twice in one call");
        seen[(size_t)slots[q]] = 1;
        if (int e = sfr_check_params(rparams + q)) return e;
        if (int e = check_track_params(tparams + q)) return e;
        if (int e = check_camera("sft", cameras + q)) return e;
        if (form == FORM_STREAMS) {
            if (int e = check_stream(h, streams[q])) return e;  // where sf_get_current / sf_get_b_image refuse, with their code
        } else {
            if (!depth[q]) return fail(SF_ERR_ARG, w + ": null depth image");
            if (rparams[q].use_b && !(b && b[q])) return fail(SF_ERR_ARG, w + ": use_b without a b image");
        }
    }
    HIP_TRY(hipSetDevice(h->device));
    // ---- layout
    const int M = t->max_tracks;
    const size_t px = (size_t)rows * cols;
    SfPlan p;
    const size_t o_args = p.take((size_t)n * sizeof(TkArgs));
    const size_t o_rsum = p.take((size_t)n * sizeof(sfr_summary));
    const size_t o_rreg = p.take((size_t)n * M * sizeof(sfr_region));
    const size_t o_lab = p.take((size_t)n * px * 4);
    const size_t o_O = p.take((size_t)n * M * M * 4);
    size_t o_sum = 0, o_trk = 0;
    std::vector<size_t> o_depth, o_b, o_ids;
    if (form != FORM_DEVICE) {
        o_sum = p.take((size_t)n * sizeof(sft_summary));
        o_trk = p.take((size_t)n * M * sizeof(sft_track));
        o_depth.assign((size_t)n, 0);
        o_b.assign((size_t)n, 0);
        o_ids.assign((size_t)n, 0);
        for (int q = 0; q < n; q++) {
            if (form == FORM_HOST) {
                o_depth[(size_t)q] = p.take(px * 4);
                if (rparams[q].use_b) o_b[(size_t)q] = p.take(px * 4);
            }
            if (ids && ids[q]) o_ids[(size_t)q] = p.take(px * 4);
        }
    }
    if (int e = t->scratch.grow(t->own, p.off, h->stream)) return e;
    unsigned char *base = t->scratch.dev;
    // ---- the frames, and the labelling as sf_regions.h has it: labels, summaries and records into the scratch
    std::vector<const void *> dp((size_t)n), bp((size_t)n);
    std::vector<void *> lp((size_t)n);
    for (int q = 0; q < n; q++) {
        const bool use_b = rparams[q].use_b != 0;
        if (form == FORM_STREAMS) {
            const size_t st = (size_t)streams[q];
            dp[(size_t)q] = h->k.pyr_new[0] + st * h->k.n_tot;  // what sf_get_current and sf_get_b_image copy out
            bp[(size_t)q] = use_b ? h->k.b_img + st * h->k.n0 : nullptr;
        } else if (form == FORM_HOST) {
            dp[(size_t)q] = base + o_depth[(size_t)q];
            bp[(size_t)q] = use_b ? base + o_b[(size_t)q] : nullptr;
            HIP_TRY(hipMemcpyAsync(base + o_depth[(size_t)q], depth[q], px * 4, hipMemcpyHostToDevice, h->stream));
            if (use_b) HIP_TRY(hipMemcpyAsync(base + o_b[(size_t)q], b[q], px * 4, hipMemcpyHostToDevice, h->stream));
        } else {
            dp[(size_t)q] = depth[q];
            bp[(size_t)q] = use_b ? b[q] : nullptr;
        }
        lp[(size_t)q] = base + o_lab + (size_t)q * px * 4;
    }
    sfr_summary *d_rsum = (sfr_summary *)(base + o_rsum);
    sfr_region *d_rreg = (sfr_region *)(base + o_rreg);
    if (int e = sfr_label_images_device(h, rows, cols, n, dp.data(), bp.data(), rparams, M, d_rsum, d_rreg, lp.data())) return e;
    // ---- the entry table
    TkArgs *tab = t->scratch.zeroed<TkArgs>((size_t)n);
    bool any_prev = false;
    for (int q = 0; q < n; q++) {
        TkArgs &a = tab[(size_t)q];
        const size_t s = (size_t)slots[q];
        const sft_params &tp = tparams[q];
        a.depth = (const float *)dp[(size_t)q];
        a.labels = (const int *)lp[(size_t)q];
        if (form == FORM_DEVICE) a.ids = ids ? (int *)ids[q] : nullptr;
        else a.ids = (ids && ids[q]) ? (int *)(base + o_ids[(size_t)q]) : nullptr;
        a.slot = t->state + s * t->lay.stride;
        a.cam = cameras[q];
        a.has_prev = t->has_prev[s];
        for (int i = 0; i < 16; i++) a.D[i] = (i % 5 == 0) ? 1.f : 0.f;
        if (a.has_prev) {
            const sft_camera &c0 = t->cams[s];
            if (int e = relative(c0.pose, cameras[q].pose, a.D)) return e;  // (both were checked: it does not fail)
            a.cx0 = c0.cx; a.cy0 = c0.cy; a.fx0 = c0.fx; a.fy0 = c0.fy;
            any_prev = true;
        }
        a.dz_abs = tp.dz_abs; a.dz_rel = tp.dz_rel;
        a.min_overlap = tp.min_overlap; a.min_share = tp.min_share; a.use_gate = tp.use_depth_gate;
    }
    const TkArgs *d_args = (const TkArgs *)(base + o_args);
    int *d_O = (int *)(base + o_O);
    sft_summary *d_sum = form == FORM_DEVICE ? (sft_summary *)summaries : (sft_summary *)(base + o_sum);
    sft_track *d_trk = form == FORM_DEVICE ? (sft_track *)tracks : (sft_track *)(base + o_trk);
    if (int e = t->scratch.upload(o_args, tab, (size_t)n * sizeof(TkArgs), h->stream)) return e;
    HIP_TRY(hipMemsetAsync(d_sum, 0, (size_t)n * sizeof(sft_summary), h->stream));
    // ---- the three launches: every grid-wide order is a launch boundary
    const unsigned un = (unsigned)n;
    if (any_prev) {
        HIP_TRY(hipMemsetAsync(d_O, 0, (size_t)n * M * M * 4, h->stream));
        hipLaunchKernelGGL(sft_overlap_kernel, dim3((unsigned)((px + SFT_PB - 1) / SFT_PB), un), dim3(SFT_NT), 0, h->stream, d_args, t->lay, rows, cols, M,
                           (const sfr_summary *)d_rsum, d_O, d_sum);
    }
    hipLaunchKernelGGL(sft_assign_kernel, dim3(un), dim3(SFT_NT), 0, h->stream, d_args, t->lay, M, (const sfr_summary *)d_rsum, (const sfr_region *)d_rreg,
                       (const int *)d_O, d_sum, d_trk);
    hipLaunchKernelGGL(sft_commit_kernel, dim3((unsigned)((px + SFT_NT - 1) / SFT_NT), un), dim3(SFT_NT), 0, h->stream, d_args, t->lay, rows, cols, M,
                       (const sfr_summary *)d_rsum, d_trk);
    HIP_TRY(hipGetLastError());
    for (int q = 0; q < n; q++) {  // what the next update of these slots warps from
        t->has_prev[(size_t)slots[q]] = 1;
        t->cams[(size_t)slots[q]] = cameras[q];
    }
    if (form == FORM_DEVICE) return SF_OK;
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(summaries, d_sum, (size_t)n * sizeof(sft_summary), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(tracks, d_trk, (size_t)n * M * sizeof(sft_track), hipMemcpyDeviceToHost));
    for (int q = 0; q < n; q++)
        if (ids && ids[q]) HIP_TRY(hipMemcpy(ids[q], base + o_ids[(size_t)q], px * 4, hipMemcpyDeviceToHost));
    return SF_OK;
}

extern "C" {

int sft_version(void) { return SFT_VERSION; }
size_t sft_camera_bytes(void) { return sizeof(sft_camera); }
size_t sft_params_bytes(void) { return sizeof(sft_params); }
size_t sft_track_bytes(void) { return sizeof(sft_track); }
size_t sft_summary_bytes(void) { return sizeof(sft_summary); }
size_t sft_info_bytes(void) { return sizeof(sft_info); }
size_t sft_slot_bytes(void) { return sizeof(sft_slot); }

int sft_default_params(sft_params *p) {
    if (!p) return fail(SF_ERR_ARG, "sft_default_params: null");
    *p = sft_params{1, 256, 1, 0.10f, 0.05f, {0, 0, 0}};
    return SF_OK;
}

int sft_check_params(const sft_params *p) { return check_track_params(p); }

int sft_relative(const float prev_pose[16], const float cur_pose[16], float d_out[16]) {
    if (!prev_pose || !cur_pose || !d_out) return fail(SF_ERR_ARG, "sft_relative: null argument");
    float D[16];
    if (int e = relative(prev_pose, cur_pose, D)) return e;
    std::memcpy(d_out, D, sizeof(D));
    return SF_OK;
}

int sft_assign(int k_prev, int k, const int32_t *overlap, const int32_t *n_prev, const int32_t *n_cur, int min_overlap, int min_share,
               int32_t *prev_of_cur_out, int32_t *cur_of_prev_out, int32_t *n_matched_out) {
    if (k_prev < 0 || k_prev > SFT_MAX_TRACKS || k < 0 || k > SFT_MAX_TRACKS) return fail(SF_ERR_ARG, "sft_assign: k_prev and k lie in 0..256");
    if ((k_prev > 0 && !n_prev) || (k > 0 && (!n_cur || !prev_of_cur_out)) || (k_prev > 0 && k > 0 && !overlap)) return fail(SF_ERR_ARG, "sft_assign: null argument");
    if (min_overlap < 1 || min_share < 0 || min_share > 1024) return fail(SF_ERR_ARG, "sft_assign: min_overlap >= 1 and min_share lies in 0..1024");
    int32_t cur_of_prev[SFT_MAX_TRACKS], prev_of_cur[SFT_MAX_TRACKS];
    const int taken = sft_assign_rounds(SftSolo(), k_prev, k, overlap, k, n_prev, n_cur, min_overlap, min_share, prev_of_cur, cur_of_prev);
    if (k > 0) std::memcpy(prev_of_cur_out, prev_of_cur, (size_t)k * 4);
    if (cur_of_prev_out && k_prev > 0) std::memcpy(cur_of_prev_out, cur_of_prev, (size_t)k_prev * 4);
    if (n_matched_out) *n_matched_out = taken;
    return SF_OK;
}

int sft_tracker_create(sf_handle *h, int rows, int cols, int n_slots, int max_tracks, sft_tracker **out) {
    if (!h || !out) return fail(SF_ERR_ARG, "sft_tracker_create: null argument");
    if (int e = check_image_size("sft_tracker_create", rows, cols)) return e;
    if (n_slots < 1 || n_slots > 65535) return fail(SF_ERR_ARG, "sft_tracker_create: n_slots lies in 1..65535");
    if (max_tracks < 1 || max_tracks > SFT_MAX_TRACKS) return fail(SF_ERR_ARG, "sft_tracker_create: max_tracks lies in 1..256");
    HIP_TRY(hipSetDevice(h->device));
    sft_tracker *t = new sft_tracker;
    t->rows = rows; t->cols = cols; t->n_slots = n_slots; t->max_tracks = max_tracks;
    t->lay = slot_layout(rows, cols, max_tracks);
    if (int e = t->own.device(&t->state, (size_t)n_slots * t->lay.stride)) {
        delete t;
        return e;
    }
    t->has_prev.assign((size_t)n_slots, 0);
    t->cams.assign((size_t)n_slots, sft_camera{});
    t->h = h;
    h->parts.enter(t);
    *out = t;
    return SF_OK;
}

void sft_tracker_destroy(sft_tracker *t) {
    if (!t) return;
    part_destroy(t);
    delete t;
}

int sft_tracker_info(const sft_tracker *t, sft_info *info_out) {
    if (int e = check_tracker("sft_tracker_info", t)) return e;
    if (!info_out) return fail(SF_ERR_ARG, "sft_tracker_info: null");
    *info_out = sft_info{t->rows, t->cols, t->n_slots, t->max_tracks, {0, 0, 0, 0}};
    return SF_OK;
}

int sft_slot_info(sft_tracker *t, int slot, sft_slot *slot_out) {
    if (int e = check_tracker("sft_slot_info", t)) return e;
    if (!slot_out) return fail(SF_ERR_ARG, "sft_slot_info: null");
    if (slot < 0 || slot >= t->n_slots) return fail(SF_ERR_ARG, "sft_slot_info: slot out of range");
    HIP_TRY(hipSetDevice(t->h->device));
    HIP_TRY(hipStreamSynchronize(t->h->stream));
    TkSlotHead head;
    HIP_TRY(hipMemcpy(&head, t->state + (size_t)slot * t->lay.stride, sizeof(head), hipMemcpyDeviceToHost));
    *slot_out = sft_slot{head.frames, head.given + 1, t->has_prev[(size_t)slot] ? head.k_prev : 0, 0};
    return SF_OK;
}

int sft_reset_slots(sft_tracker *t, int n, const int32_t *slots, int restart_ids) {
    if (int e = check_tracker("sft_reset_slots", t)) return e;
    if (int e = check_batch("sft_reset_slots", n)) return e;
    if (n == 0) return SF_OK;
    if (!slots) return fail(SF_ERR_ARG, "sft_reset_slots: null argument");
    for (int q = 0; q < n; q++)
        if (slots[q] < 0 || slots[q] >= t->n_slots) return fail(SF_ERR_ARG, "sft_reset_slots: slot out of range");
    sf_handle *h = t->h;
    HIP_TRY(hipSetDevice(h->device));
    if (int e = t->scratch.grow(t->own, (size_t)n * 4, h->stream)) return e;
    int32_t *stab = t->scratch.resized<int32_t>((size_t)n, 1);
    std::memcpy(stab, slots, (size_t)n * 4);
    if (int e = t->scratch.upload(0, stab, (size_t)n * 4, h->stream)) return e;
    hipLaunchKernelGGL(sft_reset_kernel, dim3((unsigned)((n + SFT_NT - 1) / SFT_NT)), dim3(SFT_NT), 0, h->stream, t->state, t->lay, (const int *)t->scratch.dev, n,
                       restart_ids != 0);
    HIP_TRY(hipGetLastError());
    for (int q = 0; q < n; q++) t->has_prev[(size_t)slots[q]] = 0;
    return SF_OK;
}

int sft_update_streams(sft_tracker *t, int n, const int32_t *slots, const int32_t *streams, const sft_camera *cameras, const sfr_params *rparams,
                       const sft_params *tparams, sft_summary *summaries_out, sft_track *tracks_out, int32_t *const *ids_out) {
    return update("sft_update_streams", FORM_STREAMS, t, 0, 0, n, slots, streams, nullptr, nullptr, cameras, rparams, tparams, summaries_out, tracks_out,
                  (void *const *)ids_out);
}

int sft_update_images(sft_tracker *t, int rows, int cols, int n, const int32_t *slots, const float *const *depth, const float *const *b,
                      const sft_camera *cameras, const sfr_params *rparams, const sft_params *tparams, sft_summary *summaries_out, sft_track *tracks_out,
                      int32_t *const *ids_out) {
    return update("sft_update_images", FORM_HOST, t, rows, cols, n, slots, nullptr, (const void *const *)depth, (const void *const *)b, cameras, rparams, tparams,
                  summaries_out, tracks_out, (void *const *)ids_out);
}

int sft_update_images_device(sft_tracker *t, int rows, int cols, int n, const int32_t *slots, const void *const *depth, const void *const *b,
                             const sft_camera *cameras, const sfr_params *rparams, const sft_params *tparams, void *summaries_out, void *tracks_out,
                             void *const *ids_out) {
    return update("sft_update_images_device", FORM_DEVICE, t, rows, cols, n, slots, nullptr, depth, b, cameras, rparams, tparams, summaries_out, tracks_out,
                  ids_out);
}

}  // extern "C"
