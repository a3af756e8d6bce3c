// sf_hip_closure.hip — libsf_hip.so, the interface of include/sf_closure.h (symbols sfc_*): loop-closure constraints from two
// drawings of a place, many closures per call (kernels: sf_closure.h; the rule host and device share: sf_closure_rules.h).
// A builder owns one call block (sf_call_block.h) under an owner of its own, as a deformation graph does. The two maps of
// entry q are drawn by the drawing stage of the views (sfv_plan / sfv_draw_keys of sf_hip_view.hip) as views 2q and 2q + 1
// into that block; behind the drawing layout lie the entry table (host copy 1; the view tables are copy 0), the accumulators
// and totals, the block counts of every entry and the records. The counting pass and the scan come first; the counts are
// read back and the capacity is checked; only then the writing pass runs and the records are copied out. sf_destroy of the
// handle releases the memory and leaves the builder as an empty shell. A build only reads its maps.
#include "../../include/sf_closure.h"
#include "sf_host.h"
#include "sf_closure.h"

#define SFC_VERSION 1
static_assert(sizeof(sfc_params) == 32, "include/sf_closure.h: sfc_params is 32 bytes");
static_assert(sizeof(sfc_counts) == 64 && offsetof(sfc_counts, sum_dz) == 48, "include/sf_closure.h: sfc_counts is 64 bytes");
static_assert(sizeof(sfc_record) == 32 && sizeof(SfcRecord) == 32 && sizeof(sfd_constraint) == 32 && offsetof(sfc_record, dst) == offsetof(sfd_constraint, dst) &&
                  offsetof(sfc_record, time) == offsetof(sfd_constraint, time) && offsetof(sfc_record, weight) == offsetof(sfd_constraint, weight) &&
                  offsetof(SfcRecord, dst) == offsetof(sfd_constraint, dst) && offsetof(SfcRecord, time) == offsetof(sfd_constraint, time) &&
                  offsetof(SfcRecord, weight) == offsetof(sfd_constraint, weight),
              "a record is the constraint of include/sf_deform.h");
static_assert(SFC_FOUND_BOTH == SFC_BIT_BOTH && SFC_FOUND_NEAR == SFC_BIT_NEAR && SFC_FOUND_APART == SFC_BIT_APART && SFC_FOUND_LINK == SFC_BIT_LINK &&
                  SFC_FOUND_PIN == SFC_BIT_PIN && SFC_FOUND_LINK_DROPPED == SFC_BIT_LINK_DROPPED && SFC_FOUND_PIN_DROPPED == SFC_BIT_PIN_DROPPED,
              "sf_closure_rules.h restates the bits of include/sf_closure.h");

struct SF_INTERNAL sfc_builder : SfPart {
    SfCallBlock blk;  // host copy 0: the view tables of the drawing stage; host copy 1: the entry table
    void shelled() override { blk.forget(); }
};

static int check_params(const sfc_params *p) {
    if (!p) return fail(SF_ERR_ARG, "sfc: null params");
    if (p->stride < 1 || p->stride > SFC_MAX_STRIDE) return fail(SF_ERR_ARG, "sfc: stride lies in 1..4096");
    if (p->pins < 0 || p->pins > 2) return fail(SF_ERR_ARG, "sfc: pins is 0, 1 or 2");
    if (std::isnan(p->gate_abs) || std::isnan(p->gate_rel) || std::isnan(p->min_time_gap) || std::isnan(p->w_link) || std::isnan(p->w_pin))
        return fail(SF_ERR_ARG, "sfc: NaN in sfc_params");
    if (p->gate_abs < 0.f || p->gate_rel < 0.f) return fail(SF_ERR_ARG, "sfc: a negative gate");
    if (p->w_link < 0.f || p->w_pin < 0.f) return fail(SF_ERR_ARG, "sfc: a negative weight");
    if (std::isinf(p->gate_rel) || std::isinf(p->w_link) || std::isinf(p->w_pin)) return fail(SF_ERR_ARG, "sfc: gate_rel and the weights are finite");
    if (p->min_time_gap == INFINITY) return fail(SF_ERR_ARG, "sfc: min_time_gap is finite or -inf");
    return SF_OK;
}

static SfcRule rule_of(const sfc_params &p) { return SfcRule{p.pins, p.gate_abs, p.gate_rel, p.min_time_gap, p.w_link, p.w_pin}; }

extern "C" {

int sfc_version(void) { return SFC_VERSION; }
size_t sfc_params_bytes(void) { return sizeof(sfc_params); }
size_t sfc_counts_bytes(void) { return sizeof(sfc_counts); }

int sfc_default_params(sfc_params *p) {
    if (!p) return fail(SF_ERR_ARG, "sfc_default_params: null");
    *p = sfc_params{4, 1, 0.1f, 0.05f, 0.0f, 1.0f, 1.0f, 0};
    return SF_OK;
}

int sfc_check_params(const sfc_params *p) { return check_params(p); }

int sfc_max_records(const sfv_view *view, int stride) {
    if (int e = sfv_check_view(view)) return e;
    if (stride < 1 || stride > SFC_MAX_STRIDE) return fail(SF_ERR_ARG, "sfc_max_records: stride lies in 1..4096");
    return 2 * sfc_samples_along(view->cols, stride) * sfc_samples_along(view->rows, stride);  // <= 2^25
}

int sfc_link_sample(const float *sa, const float *so, float zA, float zO, const float pose_from[16], const float pose_to[16], const sfc_params *params,
                    sfc_record out[2], int32_t *n_out) {
    if (!pose_from || !pose_to || !out || !n_out) return fail(SF_ERR_ARG, "sfc_link_sample: null argument");
    if (int e = check_params(params)) return e;
    if (!finite_all(pose_from, 16) || !finite_all(pose_to, 16)) return fail(SF_ERR_ARG, "sfc_link_sample: NaN or inf in a pose");
    float t_inv[16];
    invert_pose(pose_from, t_inv);
    const SfcRule r = rule_of(*params);
    SfcRecord link, pin;
    long long q_dz, q_shift;
    const int mask = sfc_link_core(sa != nullptr, sa, so != nullptr, so, zA, zO, t_inv, pose_to, &r, &link, &pin, &q_dz, &q_shift);
    int k = 0;
    if (mask & SFC_BIT_LINK) std::memcpy(out + k++, &link, sizeof(link));
    if (mask & SFC_BIT_PIN) std::memcpy(out + k++, &pin, sizeof(pin));
    *n_out = k;
    return mask;
}

int sfc_builder_create(sf_handle *h, sfc_builder **out) {
    if (!h || !out) return fail(SF_ERR_ARG, "sfc_builder_create: null argument");
    if (int e = check_live_handle("sfc_builder_create", h)) return e;
    sfc_builder *b = new sfc_builder;
    b->h = h;
    h->parts.enter(b);
    *out = b;
    return SF_OK;
}

void sfc_builder_destroy(sfc_builder *b) {
    if (!b) return;
    part_destroy(b);
    delete b;
}

// every check of the refusal list, then: plan, grow, upload, draw, count, scan, the counts, the capacity, write, the records
int sfc_build(sfc_builder *b, int n, sf_map *const *maps_new, sf_map *const *maps_old, const sfv_view *views_from, const sfv_view *views_to,
              const sfc_params *params, sfc_record *out, int max_records, sfc_counts *counts_out) {
    const std::string w("sfc_build");
    if (int e = check_part("sfc_build", b, "builder")) return e;
    sf_handle *h = b->h;
    if (n < 0) return fail(SF_ERR_ARG, w + ": n < 0");
    if (2 * (long long)n > 65535) return fail(SF_ERR_ARG, w + ": more than 65535 views in one call (two per entry)");
    if (max_records < 0 || (!out && max_records > 0)) return fail(SF_ERR_ARG, w + ": out is null with max_records > 0, or max_records < 0");
    if (n == 0) return SF_OK;
    if (!maps_new || !maps_old || !views_from || !views_to || !params || !counts_out) return fail(SF_ERR_ARG, w + ": null argument");
    std::vector<ViewJob> jobs(2 * (size_t)n);
    std::vector<sfv_view> views(2 * (size_t)n);
    for (int q = 0; q < n; q++) {
        if (int e = check_map("sfc_build", h, maps_new[q])) return e;
        if (int e = check_map("sfc_build", h, maps_old[q])) return e;
        const sfv_view &vf = views_from[q], &vt = views_to[q];
        if (int e = sfv_check_view(&vf)) return e;
        if (int e = sfv_check_view(&vt)) return e;
        if (vf.rows != vt.rows || vf.cols != vt.cols || std::memcmp(&vf.cx, &vt.cx, 4 * sizeof(float)) != 0)
            return fail(SF_ERR_ARG, w + ": the two views of an entry differ in size or intrinsics");
        if (int e = check_params(params + q)) return e;
        jobs[2 * (size_t)q] = ViewJob{maps_new[q]->buf[0], maps_new[q]->count, maps_new[q]->tick};
        jobs[2 * (size_t)q + 1] = ViewJob{maps_old[q]->buf[0], maps_old[q]->count, maps_old[q]->tick};
        views[2 * (size_t)q] = vf;
        views[2 * (size_t)q + 1] = vt;
    }
    HIP_TRY(hipSetDevice(h->device));
    // ---- layout: the drawing stage, then what the kernels here read and write
    std::vector<int> nx((size_t)n), samples((size_t)n);
    std::vector<size_t> bc_first((size_t)n);
    size_t n_blocks = 0;
    long long bound = 0;  // records the call can make at most
    int max_samples = 0;
    for (int q = 0; q < n; q++) {
        nx[(size_t)q] = sfc_samples_along(views_from[q].cols, params[q].stride);
        samples[(size_t)q] = nx[(size_t)q] * sfc_samples_along(views_from[q].rows, params[q].stride);  // <= 2^24
        bc_first[(size_t)q] = n_blocks;
        n_blocks += ((size_t)samples[(size_t)q] + SFC_NT - 1) / SFC_NT;
        bound += 2ll * samples[(size_t)q];
        max_samples = std::max(max_samples, samples[(size_t)q]);
    }
    const size_t room = (size_t)std::min<long long>(bound, max_records);  // records the device buffer holds
    ViewPlan p;
    sfv_plan(p, 2 * n, jobs.data(), views.data(), 0);
    const size_t tab_bytes = (size_t)n * sizeof(ClosureArgs);
    const size_t o_ctab = p.take(tab_bytes);
    const size_t acc_bytes = (size_t)n * SFC_FIELDS * sizeof(long long), total_bytes = (size_t)n * sizeof(int);
    const size_t o_acc = p.take(acc_bytes);
    const size_t o_total = p.take(total_bytes);
    const size_t o_bc = p.take(n_blocks * sizeof(int));
    const size_t o_out = p.take(room * sizeof(SfcRecord));
    if (int e = b->blk.grow(b->own, p.off, h->stream)) return e;
    unsigned char *base = b->blk.dev;
    // ---- the entry table (host copy 1)
    ClosureArgs *tab = b->blk.zeroed<ClosureArgs>((size_t)n, 1);
    for (int q = 0; q < n; q++) {
        ClosureArgs &a = tab[(size_t)q];
        a.stride = params[q].stride;
        a.nx = nx[(size_t)q];
        a.n_samples = samples[(size_t)q];
        a.first = 0;
        a.capacity = 0;
        a.rule = rule_of(params[q]);
        std::memcpy(a.pose_to, views_to[q].pose, sizeof(a.pose_to));
        a.block_counts = (int *)(base + o_bc) + bc_first[(size_t)q];
        a.total = (int *)(base + o_total) + q;
        a.acc = (long long *)(base + o_acc) + (size_t)q * SFC_FIELDS;
        a.out = (SfcRecord *)(base + o_out);
    }
    if (int e = b->blk.upload(o_ctab, tab, tab_bytes, h->stream)) return e;
    HIP_TRY(hipMemsetAsync(base + o_acc, 0, acc_bytes, h->stream));
    // ---- draw the keys of the 2n views, count, scan
    if (int e = sfv_draw_keys(h, p, jobs.data(), views.data(), nullptr, b->blk, nullptr, 0)) return e;
    const ViewArgs *d_vtab = (const ViewArgs *)(base + p.o_tab);
    const ClosureArgs *d_ctab = (const ClosureArgs *)(base + o_ctab);
    const dim3 grid((unsigned)((max_samples + SFC_NT - 1) / SFC_NT), (unsigned)n);
    if (max_samples) hipLaunchKernelGGL(sfc_sample_kernel<false>, grid, dim3(SFC_NT), 0, h->stream, d_vtab, d_ctab);
    hipLaunchKernelGGL(sfc_scan_kernel, dim3((unsigned)n), dim3(1024), 0, h->stream, d_ctab);
    HIP_TRY(hipGetLastError());
    // ---- the counts
    std::vector<long long> acc((size_t)n * SFC_FIELDS);
    std::vector<int> totals((size_t)n);
    if (int e = d2h(h, acc.data(), base + o_acc, acc_bytes)) return e;
    if (int e = d2h(h, totals.data(), base + o_total, total_bytes)) return e;
    long long total = 0;
    for (int q = 0; q < n; q++) {
        const long long *v = acc.data() + (size_t)q * SFC_FIELDS;
        for (int f = 0; f < 8; f++)
            if (v[f] < 0 || v[f] > 2ll * samples[(size_t)q]) return fail(SF_ERR_DEVICE, w + ": a count outside the samples came back");
        if (totals[(size_t)q] != v[5] + v[6]) return fail(SF_ERR_DEVICE, w + ": the scan and the counts disagree");
        total += totals[(size_t)q];
    }
    if (total > 0x7fffffffll) return fail(SF_ERR_ARG, w + ": more than 2^31 - 1 records in one call");
    long long first = 0;
    for (int q = 0; q < n; q++) {
        const long long *v = acc.data() + (size_t)q * SFC_FIELDS;
        sfc_counts c{};
        c.n_samples = samples[(size_t)q];
        c.n_new = (int32_t)v[0]; c.n_old = (int32_t)v[1]; c.n_both = (int32_t)v[2]; c.n_near = (int32_t)v[3]; c.n_apart = (int32_t)v[4];
        c.n_links = (int32_t)v[5]; c.n_pins = (int32_t)v[6]; c.n_dropped = (int32_t)v[7];
        c.first = (int32_t)first;
        c.sum_dz = v[8];
        c.sum_shift = v[9];
        counts_out[q] = c;
        tab[(size_t)q].first = (int)first;
        tab[(size_t)q].capacity = (int)total;
        first += totals[(size_t)q];
    }
    if (!out && max_records == 0) return SF_OK;  // the sizes were asked for
    if (total > max_records)
        return fail(SF_ERR_ARG, w + ": " + std::to_string(total) + " records, room for " + std::to_string(max_records));
    if (total == 0) return SF_OK;
    // ---- the capacity holds: write, in sample order, and copy out
    if (int e = b->blk.upload(o_ctab, tab, tab_bytes, h->stream)) return e;
    hipLaunchKernelGGL(sfc_sample_kernel<true>, grid, dim3(SFC_NT), 0, h->stream, d_vtab, d_ctab);
    HIP_TRY(hipGetLastError());
    return d2h(h, out, base + o_out, (size_t)total * sizeof(SfcRecord));
}

}  // extern "C"
