// sf_hip_register.hip — libsf_hip.so, the interface of include/sf_register.h (symbols sfg_*): surfel maps registered against each
// other on the voxel tables of their destinations, many (destination, source, start) entries per call (kernels: sf_register.h;
// the rules host and device share: sf_register_rules.h; the table and its insert kernel: sf_voxel_table.h; the system:
// sf_p2p_system.h; the step: sf_align_step.h; the state of an entry and the step's bookkeeping: sf_p2p_device.h).
// A registrar owns one call block (sf_call_block.h) under an owner of its own, as a carver does. In it lie, in one piece and
// one upload, the JoinArgs of the distinct tables and the entry table; then what is cleared to 0 (the tables' counters and bids,
// the entries' counters, results and systems), what is cleared to ~0 (the keys), and the rest (the slots the insert remembers, the
// states, the pairs). The launches are: init, insert, and per iteration and once more linearise and step; nothing is read in
// between. One host synchronisation then reads results and counters; systems and pairs follow where asked for. sf_destroy of the
// handle releases the memory and leaves the registrar as an empty shell.
#include <map>

#include "../../include/sf_register.h"
#include "sf_host.h"
#include "sf_register.h"

#define SFG_VERSION 1
static_assert(sizeof(sfg_params) == 32, "include/sf_register.h: sfg_params is 32 bytes");
static_assert(sizeof(sfg_system) == p2p::WORDS * sizeof(int64_t) && offsetof(sfg_system, reserved) == p2p::FIELDS * sizeof(int64_t),
              "include/sf_register.h: sfg_system is the system of sf_p2p_system.h, its summed words first");
static_assert(sizeof(sfg_result) == 128, "include/sf_register.h: sfg_result is 128 bytes");
static_assert(SFG_OK == p2p::OK && SFG_FEW_PAIRS == p2p::FEW_PAIRS && SFG_DEGENERATE == p2p::DEGENERATE, "include/sf_register.h: the status codes of sf_p2p_system.h");
static_assert(sizeof(RegArgs) % 8 == 0 && sizeof(JoinArgs) % 8 == 0, "the two tables follow one another aligned");

struct SF_INTERNAL sfg_registrar : SfPart {
    SfCallBlock blk;  // host copy 0: the two tables; host copy 1: what is read back
    void shelled() override { blk.forget(); }
};

static int check_params(const sfg_params *p) {
    if (!p) return fail(SF_ERR_ARG, "sfg: null params");
    if (!(std::isfinite(p->cell) && p->cell > 0.f)) return fail(SF_ERR_ARG, "sfg: cell is finite and > 0");
    if (!std::isfinite(1.0f / p->cell)) return fail(SF_ERR_ARG, "sfg: 1 / cell is not finite");
    if (!(p->dist_max > 0.f && p->dist_max <= 1.f)) return fail(SF_ERR_ARG, "sfg: dist_max lies in (0, 1]");
    if (!(p->dist_max <= 0.5f * p->cell)) return fail(SF_ERR_ARG, "sfg: dist_max is at most half a cell");
    if (!(p->min_cos >= -1.f && p->min_cos <= 1.f)) return fail(SF_ERR_ARG, "sfg: min_cos lies in [-1, 1]");
    if (std::isnan(p->min_confidence)) return fail(SF_ERR_ARG, "sfg: NaN min_confidence");
    if (!(std::isfinite(p->damping) && p->damping >= 0.f)) return fail(SF_ERR_ARG, "sfg: damping is finite and >= 0");
    if (p->iterations < 1 || p->iterations > 64) return fail(SF_ERR_ARG, "sfg: iterations lies in 1..64");
    if (p->stride < 1) return fail(SF_ERR_ARG, "sfg: stride is at least 1");
    if (p->min_pairs < 6) return fail(SF_ERR_ARG, "sfg: min_pairs is at least 6");
    return SF_OK;
}

static SfgRule rule_of(const sfg_params &p) { return SfgRule{1.0f / p.cell, p.dist_max, p.min_cos, p.min_confidence, p.min_confidence > 0.f, p.stride}; }

// the surfels e % stride == 0 of `count`
static long long strided(int count, int stride) { return ((long long)count + stride - 1) / stride; }

extern "C" {

int sfg_version(void) { return SFG_VERSION; }
size_t sfg_params_bytes(void) { return sizeof(sfg_params); }
size_t sfg_system_bytes(void) { return sizeof(sfg_system); }
size_t sfg_result_bytes(void) { return sizeof(sfg_result); }

int sfg_default_params(sfg_params *p) {
    if (!p) return fail(SF_ERR_ARG, "sfg_default_params: null");
    *p = sfg_params{0.1f, 0.05f, 0.5f, 0.0f, 0.0f, 10, 1, 64};
    return SF_OK;
}

int sfg_check_params(const sfg_params *p) { return check_params(p); }

int sfg_linearise(const float *dst, int dst_count, const float *src, int src_count, const sfg_params *params, const double E[12], sfg_system *system_out,
                  int32_t *pairs_out) {
    if (!E || !system_out || dst_count < 0 || src_count < 0 || (!dst && dst_count) || (!src && src_count)) return fail(SF_ERR_ARG, "sfg_linearise: bad argument");
    if (dst_count > SFJ_MAX_COUNT || src_count > SFJ_MAX_COUNT) return fail(SF_ERR_ARG, "sfg_linearise: a count lies in 0 .. 2^29");
    if (int e = check_params(params)) return e;
    float Ef[12];
    for (int k = 0; k < 12; k++) {
        if (!std::isfinite(E[k])) return fail(SF_ERR_ARG, "sfg_linearise: NaN or inf in E");
        Ef[k] = (float)E[k];
    }
    if (strided(src_count, params->stride) > SFG_MAX_SAMPLED) return fail(SF_ERR_ARG, "sfg_linearise: more than 2^24 sampled surfels");
    const SfgRule rule = rule_of(*params);
    SfgHostTable t;
    t.surfels = dst;
    t.count = dst_count;
    t.slots = sfj_slots_for(dst_count);
    t.log2_slots = sfj_log2_of(t.slots);
    std::vector<uint64_t> words(2 * (size_t)t.slots);
    t.keys = words.data();
    t.bids = words.data() + t.slots;
    if (!sfg_fill_host(&t, rule.inv)) return fail(SF_ERR_STATE, "sfg_linearise: a probe walk visited every slot of the table");
    long long w[SFG_SYSTEM_WORDS];
    int n_sampled = 0, n_outside = 0;
    std::vector<int32_t> pairs(pairs_out ? (size_t)src_count : 0);
    if (!sfg_linearise_host(t, rule, Ef, src, src_count, w, &n_sampled, &n_outside, pairs_out ? pairs.data() : nullptr))
        return fail(SF_ERR_STATE, "sfg_linearise: a probe walk visited every slot of the table");
    std::memcpy(system_out, w, sizeof(sfg_system));
    if (pairs_out && src_count) std::memcpy(pairs_out, pairs.data(), (size_t)src_count * sizeof(int32_t));
    return SF_OK;
}

int sfg_registrar_create(sf_handle *h, sfg_registrar **out) {
    if (!h || !out) return fail(SF_ERR_ARG, "sfg_registrar_create: null argument");
    if (int e = check_live_handle("sfg_registrar_create", h)) return e;
    sfg_registrar *r = new sfg_registrar;
    r->h = h;
    h->parts.enter(r);
    *out = r;
    return SF_OK;
}

void sfg_registrar_destroy(sfg_registrar *reg) {
    if (!reg) return;
    part_destroy(reg);
    delete reg;
}

int sfg_register_maps(sfg_registrar *reg, int n, sf_map *const *dst, sf_map *const *src, const float *T0, const sfg_params *params, sfg_result *results,
                      sfg_system *systems_out, int32_t *const *pairs_out) {
    const char *what = "sfg_register_maps";
    const std::string w(what);
    if (int e = check_part(what, reg, "registrar")) return e;
    sf_handle *h = reg->h;
    if (int e = check_batch(w, n)) return e;
    if (n == 0) return SF_OK;
    if (!dst || !src || !params || !results) return fail(SF_ERR_ARG, w + ": null argument");
    int I = 0;
    for (int q = 0; q < n; q++) {
        if (int e = check_map(what, h, dst[q])) return e;
        if (int e = check_map(what, h, src[q])) return e;
        if (dst[q] == src[q]) return fail(SF_ERR_ARG, w + ": a map registered against itself");
        if (int e = check_params(params + q)) return e;
        if (T0 && !finite_all(T0 + (size_t)q * 16, 16)) return fail(SF_ERR_ARG, w + ": NaN or inf in T0");
        if (strided(src[q]->count, params[q].stride) > SFG_MAX_SAMPLED) return fail(SF_ERR_ARG, w + ": more than 2^24 sampled surfels in an entry");
        I = std::max(I, params[q].iterations);
    }
    HIP_TRY(hipSetDevice(h->device));
    // ---- the distinct tables: (destination, cell) in the order of their first entry
    std::vector<int> table_of((size_t)n), first_entry;
    std::map<std::pair<const sf_map *, uint32_t>, int> seen;
    for (int q = 0; q < n; q++) {
        uint32_t cell_bits;
        std::memcpy(&cell_bits, &params[q].cell, sizeof(float));
        const auto at = seen.emplace(std::make_pair((const sf_map *)dst[q], cell_bits), (int)first_entry.size());
        if (at.second) first_entry.push_back(q);
        table_of[(size_t)q] = at.first->second;
    }
    const int nt = (int)first_entry.size();
    const int keep = systems_out ? 1 : 0, sys_slots = keep ? I + 1 : 1;
    // ---- layout
    SfPlan p;
    const size_t jtab_bytes = (size_t)nt * sizeof(JoinArgs), etab_bytes = (size_t)n * sizeof(RegArgs), tab_bytes = jtab_bytes + etab_bytes;
    const size_t o_tab = p.take(tab_bytes);
    p.zeros_from_here();
    // what is read back, in one piece: the results, the entries' counters, the tables' counters
    const size_t res_bytes = (size_t)n * sizeof(sfg_result), ecount_bytes = (size_t)n * SFG_COUNT_WORDS * sizeof(int), tcount_bytes = (size_t)nt * SFJ_COUNT_WORDS * sizeof(int);
    const size_t back_bytes = res_bytes + ecount_bytes + tcount_bytes;
    const size_t o_back = p.take(back_bytes);
    const size_t sys_bytes = (size_t)n * sys_slots * sizeof(sfg_system);
    const size_t o_sys = p.take(sys_bytes);
    std::vector<size_t> o_best((size_t)nt), o_keys((size_t)nt), o_slot((size_t)nt), o_pairs((size_t)n);
    std::vector<int> slots((size_t)nt);
    int max_fill = 0, max_total = 0;
    for (int t = 0; t < nt; t++) {
        const int count = dst[first_entry[(size_t)t]]->count;
        slots[(size_t)t] = sfj_slots_for(count);
        o_best[(size_t)t] = p.take((size_t)slots[(size_t)t] * 8);
        max_fill = std::max(max_fill, count);
    }
    p.ones_from_here();
    for (int t = 0; t < nt; t++) o_keys[(size_t)t] = p.take((size_t)slots[(size_t)t] * 8);
    p.rest_from_here();
    for (int t = 0; t < nt; t++) o_slot[(size_t)t] = p.take((size_t)dst[first_entry[(size_t)t]]->count * sizeof(int));
    const size_t o_state = p.take((size_t)n * sizeof(P2pState));
    std::vector<int> total((size_t)n);
    for (int q = 0; q < n; q++) {
        total[(size_t)q] = (int)strided(src[q]->count, params[q].stride);
        max_total = std::max(max_total, total[(size_t)q]);
        if (pairs_out && pairs_out[q]) o_pairs[(size_t)q] = p.take((size_t)total[(size_t)q] * sizeof(int));
    }
    if (int e = reg->blk.grow(reg->own, p.off, h->stream)) return e;
    unsigned char *base = reg->blk.dev;
    // ---- the tables (host copy 0): one upload
    unsigned char *tabs = reg->blk.zeroed<unsigned char>(tab_bytes);
    JoinArgs *jtab = (JoinArgs *)tabs;
    RegArgs *etab = (RegArgs *)(tabs + jtab_bytes);
    int *d_tcounts = (int *)(base + o_back + res_bytes + ecount_bytes);
    for (int t = 0; t < nt; t++) {
        const int f = first_entry[(size_t)t];
        JoinArgs &a = jtab[(size_t)t];
        a.fill = a.src = dst[f]->buf[0];
        a.fill_count = a.count = dst[f]->count;
        a.slots = slots[(size_t)t];
        a.log2_slots = sfj_log2_of(a.slots);
        a.inv = 1.0f / params[f].cell;
        a.stamp = -1;
        a.keys = (unsigned long long *)(base + o_keys[(size_t)t]);
        a.best = (unsigned long long *)(base + o_best[(size_t)t]);
        a.slot_of = (int *)(base + o_slot[(size_t)t]);
        a.counts = d_tcounts + (size_t)t * SFJ_COUNT_WORDS;
    }
    for (int q = 0; q < n; q++) {
        RegArgs &a = etab[(size_t)q];
        a.src = src[q]->buf[0];
        a.count = src[q]->count;
        a.total = total[(size_t)q];
        a.table = table_of[(size_t)q];
        a.rule = rule_of(params[q]);
        a.damping = params[q].damping;
        a.iterations = params[q].iterations;
        a.min_pairs = params[q].min_pairs;
        for (int k = 0; k < 16; k++) a.T0[k] = T0 ? T0[(size_t)q * 16 + k] : (k % 5 == 0 ? 1.f : 0.f);
        a.systems = (long long *)(base + o_sys) + (size_t)q * sys_slots * SFG_SYSTEM_WORDS;
        a.state = (P2pState *)(base + o_state) + q;
        a.result = (sfg_result *)(base + o_back) + q;
        a.counts = (int *)(base + o_back + res_bytes) + (size_t)q * SFG_COUNT_WORDS;
        a.pairs = (pairs_out && pairs_out[q]) ? (int *)(base + o_pairs[(size_t)q]) : nullptr;
    }
    if (int e = reg->blk.upload(o_tab, tabs, tab_bytes, h->stream)) return e;
    if (int e = p.clear(base, h->stream)) return e;
    const JoinArgs *dj = (const JoinArgs *)(base + o_tab);
    const RegArgs *de = (const RegArgs *)(base + o_tab + jtab_bytes);
    // ---- init, insert, then linearise and step I + 1 times
    const unsigned entry_blocks = (unsigned)((n + 63) / 64);
    hipLaunchKernelGGL(sfg_init_kernel, dim3(entry_blocks), dim3(64), 0, h->stream, de, n);
    if (max_fill) hipLaunchKernelGGL(sfj_insert_kernel<true>, dim3((unsigned)((max_fill + SFJ_BLOCK - 1) / SFJ_BLOCK), (unsigned)nt), dim3(SFJ_BLOCK), 0, h->stream, dj);
    for (int it = 0; it <= I; it++) {
        const int slot = keep ? it : 0;
        if (max_total)
            hipLaunchKernelGGL(sfg_linearise_kernel, dim3((unsigned)((max_total + SFG_PER_BLOCK - 1) / SFG_PER_BLOCK), (unsigned)n), dim3(SFG_NT), 0, h->stream, dj, de,
                               slot, it);
        hipLaunchKernelGGL(sfg_step_kernel, dim3(entry_blocks), dim3(64), 0, h->stream, de, n, slot, keep, it);
    }
    HIP_TRY(hipGetLastError());
    // ---- results and counters, once
    unsigned char *back = reg->blk.resized<unsigned char>(back_bytes, 1);
    if (int e = d2h(h, back, base + o_back, back_bytes)) return e;
    const int *ecounts = (const int *)(back + res_bytes), *tcounts = (const int *)(back + res_bytes + ecount_bytes);
    for (int t = 0; t < nt; t++)
        if (tcounts[(size_t)t * SFJ_COUNT_WORDS + SFJ_ERROR]) return fail(SF_ERR_STATE, w + ": a probe walk visited every slot of a table");
    for (int q = 0; q < n; q++)
        if (ecounts[(size_t)q * SFG_COUNT_WORDS + SFG_ERROR]) return fail(SF_ERR_STATE, w + ": a probe walk visited every slot of a table");
    if (systems_out) HIP_TRY(hipMemcpy(systems_out, base + o_sys, sys_bytes, hipMemcpyDeviceToHost));
    if (pairs_out) {
        std::vector<int> packed;
        for (int q = 0; q < n; q++) {
            if (!pairs_out[q] || src[q]->count == 0) continue;
            packed.resize((size_t)total[(size_t)q]);
            HIP_TRY(hipMemcpy(packed.data(), base + o_pairs[(size_t)q], packed.size() * sizeof(int), hipMemcpyDeviceToHost));
            const int stride = params[q].stride;
            for (int e = 0; e < src[q]->count; e++) pairs_out[q][e] = e % stride == 0 ? packed[(size_t)(e / stride)] : SFG_NOT_SAMPLED;
        }
    }
    std::memcpy(results, back, res_bytes);
    return SF_OK;
}

}  // extern "C"
