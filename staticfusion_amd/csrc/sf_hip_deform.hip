// sf_hip_deform.hip — libsf_hip.so, the interface of include/sf_deform.h (symbols sfd_*): surfel maps bent by a deformation
// graph, many per call (kernel: sf_deform.h; the rules host and device share: sf_deform_rules.h; the solver: sf_deform_solve.h).
// A graph owns one call block (sf_call_block.h) under an owner of its own, as a keyframe database does: host copy 0 is the
// graph itself -- (g, time) of every node, then the transforms --, and a call that uses the graph lays out in the device
// block the nodes, which it uploads anew (the contents of a block do not survive a call), and behind them what the call's
// entries under this graph write: bindings or per-workgroup counts. The entry table of a call lies in the block of the graph
// of entry 0 (host copy 1). sf_destroy of the handle releases the memory and leaves the graph as an empty shell. The node
// sampling calls the thinning of include/sf_join.h. One host synchronisation per entry reads the results.
#include "../../include/sf_deform.h"
#include "../../include/sf_join.h"
#include "sf_host.h"
#include "sf_deform.h"
#include "sf_deform_solve.h"

#define SFD_VERSION 1
static_assert(sizeof(sfd_params) == 32, "include/sf_deform.h: sfd_params is 32 bytes");
static_assert(sizeof(sfd_counts) == 32, "include/sf_deform.h: sfd_counts is 32 bytes");
static_assert(sizeof(sfd_info) == 16, "include/sf_deform.h: sfd_info is 16 bytes");
static_assert(sizeof(sfd_constraint) == 32 && sizeof(SfdConstraint) == 32 && offsetof(sfd_constraint, dst) == offsetof(SfdConstraint, dst) &&
                  offsetof(sfd_constraint, time) == offsetof(SfdConstraint, time) && offsetof(sfd_constraint, weight) == offsetof(SfdConstraint, weight),
              "include/sf_deform.h: sfd_constraint is 32 bytes, the constraint of sf_deform_solve.h");
static_assert(sizeof(sfd_solve_params) == 32, "include/sf_deform.h: sfd_solve_params is 32 bytes");
static_assert(sizeof(sfd_report) == 280 && offsetof(sfd_report, energy) == 16, "include/sf_deform.h: sfd_report is 280 bytes");
static_assert(SFD_SOLVE_MAX_ITERATIONS == SFD_MAX_ITERATIONS && SFD_SOLVE_MAX_NODES <= SFD_MAX_NODES && SFD_SOLVE_OK == SFD_OK &&
                  SFD_SOLVE_DEGENERATE == SFD_DEGENERATE,
              "sf_deform_solve.h restates the constants of include/sf_deform.h");

struct SF_INTERNAL sfd_graph : SfPart {
    int max_nodes = 0, G = 0;
    SfCallBlock blk;  // host copy 0: G x 4 floats (g, time), then G x 12 (M); host copy 1: the entry table of a call
    void shelled() override { blk.forget(); }
};

static int check_params(const sfd_params *p) {
    if (!p) return fail(SF_ERR_ARG, "sfd: null params");
    if (!(p->time_window >= 0.f)) return fail(SF_ERR_ARG, "sfd: time_window is >= 0 (+inf allowed), not NaN");
    return SF_OK;
}

static int check_solve_params(const sfd_solve_params *p) {
    if (!p) return fail(SF_ERR_ARG, "sfd: null solve params");
    if (!(p->time_window >= 0.f)) return fail(SF_ERR_ARG, "sfd: time_window is >= 0 (+inf allowed), not NaN");
    if (!(std::isfinite(p->w_reg) && p->w_reg >= 0.f)) return fail(SF_ERR_ARG, "sfd: w_reg is finite and >= 0");
    if (!(std::isfinite(p->damping) && p->damping >= 0.f)) return fail(SF_ERR_ARG, "sfd: damping is finite and >= 0");
    if (p->iterations < 1 || p->iterations > SFD_MAX_ITERATIONS) return fail(SF_ERR_ARG, "sfd: iterations lies in 1..32");
    return SF_OK;
}

static int check_graph(const char *what, const sfd_graph *g) { return check_part(what, g, "graph"); }

// the arguments of the pure-host calls that take a graph as arrays
static int check_arrays(const std::string &w, int G, int max_G, const float *pos, const float *times, const float *M, bool need_M, float time_window) {
    if (G < 1 || G > max_G) return fail(SF_ERR_ARG, w + ": G lies in 1.." + std::to_string(max_G));
    if (!pos || !times || (need_M && !M)) return fail(SF_ERR_ARG, w + ": null argument");
    if (!(time_window >= 0.f)) return fail(SF_ERR_ARG, w + ": time_window is >= 0 (+inf allowed), not NaN");
    if (M && !finite_all(M, 12 * G)) return fail(SF_ERR_ARG, w + ": NaN or inf in M");
    return SF_OK;
}

// sfd_bind_maps (apply false) and sfd_apply_maps: every check of the refusal list, then per distinct graph the layout of its
// block, the growth of all of them, the uploads, one launch, the results.
static int run(const char *what, bool apply, sf_handle *h, int n, sf_map *const *maps, sfd_graph *const *graphs, const sfd_params *params, int32_t *idx_out,
               float *w_out, sfd_counts *counts_out) {
    const std::string w(what);
    if (!h || n < 0) return fail(SF_ERR_ARG, w + ": bad argument");
    if (int e = check_live_handle(w, h)) return e;
    if (n == 0) return SF_OK;
    if (int e = check_batch(w, n)) return e;
    if (!maps || !graphs || !params || (apply ? !counts_out : (!idx_out || !w_out))) return fail(SF_ERR_ARG, w + ": null argument");
    for (int q = 0; q < n; q++) {
        if (int e = check_map(what, h, maps[q])) return e;
        if (int e = check_distinct(w, maps, q, "the same map twice in one call")) return e;
        if (int e = check_graph(what, graphs[q])) return e;
        if (graphs[q]->h != h) return fail(SF_ERR_ARG, w + ": a graph of another handle");
        if (graphs[q]->G == 0) return fail(SF_ERR_STATE, w + ": a graph without nodes");
        if (int e = check_params(params + q)) return e;
    }
    HIP_TRY(hipSetDevice(h->device));
    // ---- layout, graph by graph in the order of their first entry
    std::vector<sfd_graph *> used;
    std::vector<SfPlan> plans;
    std::vector<int> graph_of((size_t)n);
    std::vector<size_t> o_res((size_t)n), o_w((size_t)n);
    size_t o_tab = 0;
    const size_t tab_bytes = (size_t)n * sizeof(DeformArgs);
    int max_count = 0;
    for (int q = 0; q < n; q++) {
        size_t u = std::find(used.begin(), used.end(), graphs[q]) - used.begin();
        if (u == used.size()) {
            used.push_back(graphs[q]);
            plans.emplace_back();
            plans[u].take((size_t)graphs[q]->G * 64);  // the nodes, at offset 0
            if (q == 0) o_tab = plans[u].take(tab_bytes);
        }
        graph_of[(size_t)q] = (int)u;
        const size_t count = (size_t)maps[q]->count, blocks = (count + SFD_BLOCK - 1) / SFD_BLOCK;
        if (apply) {
            o_res[(size_t)q] = plans[u].take(blocks * 2 * sizeof(int));
        } else {
            o_res[(size_t)q] = plans[u].take(count * 4 * sizeof(int));
            o_w[(size_t)q] = plans[u].take(count * 4 * sizeof(float));
        }
        max_count = std::max(max_count, maps[q]->count);
    }
    for (size_t u = 0; u < used.size(); u++)
        if (int e = used[u]->blk.grow(used[u]->own, plans[u].off, h->stream)) return e;
    // ---- the nodes of every graph and the entry table
    for (size_t u = 0; u < used.size(); u++)
        if (int e = used[u]->blk.upload(0, used[u]->blk.host[0].data(), (size_t)used[u]->G * 64, h->stream)) return e;
    sfd_graph *g0 = used[0];
    DeformArgs *tab = g0->blk.zeroed<DeformArgs>((size_t)n, 1);
    for (int q = 0; q < n; q++) {
        sfd_graph *g = graphs[q];
        unsigned char *base = g->blk.dev;
        DeformArgs &a = tab[(size_t)q];
        a.map = maps[q]->buf[0];
        a.count = maps[q]->count;
        a.G = g->G;
        a.nodes = (const vfloat4 *)base;
        a.M = (const float *)(base + (size_t)g->G * 16);
        a.time_window = params[q].time_window;
        if (apply) {
            a.block_counts = (int *)(base + o_res[(size_t)q]);
        } else {
            a.idx_out = (int *)(base + o_res[(size_t)q]);
            a.w_out = (float *)(base + o_w[(size_t)q]);
        }
    }
    if (int e = g0->blk.upload(o_tab, tab, tab_bytes, h->stream)) return e;
    const DeformArgs *d_tab = (const DeformArgs *)(g0->blk.dev + o_tab);
    if (max_count) {
        const dim3 grid((unsigned)((max_count + SFD_BLOCK - 1) / SFD_BLOCK), (unsigned)n);
        if (apply)
            hipLaunchKernelGGL(sfd_kernel<true>, grid, dim3(SFD_BLOCK), 0, h->stream, d_tab);
        else
            hipLaunchKernelGGL(sfd_kernel<false>, grid, dim3(SFD_BLOCK), 0, h->stream, d_tab);
    }
    HIP_TRY(hipGetLastError());
    if (apply)
        for (int q = 0; q < n; q++) indices_moved(maps[q]);
    // ---- the results
    size_t first = 0;  // bind: surfels of the entries before
    std::vector<int> bc;
    for (int q = 0; q < n; q++) {
        const size_t count = (size_t)maps[q]->count, blocks = (count + SFD_BLOCK - 1) / SFD_BLOCK;
        if (apply) {
            bc.assign(blocks * 2, 0);
            if (blocks)
                if (int e = d2h(h, bc.data(), tab[(size_t)q].block_counts, blocks * 2 * sizeof(int))) return e;
            long long bound = 0, few = 0;
            for (size_t b = 0; b < blocks; b++) {
                bound += bc[2 * b];
                few += bc[2 * b + 1];
            }
            if (bound < 0 || bound > (long long)count || few < 0 || few > bound) return fail(SF_ERR_DEVICE, w + ": a count outside the map came back");
            sfd_counts c{};
            c.n_surfels = (int32_t)count;
            c.n_bound = (int32_t)bound;
            c.n_unbound = (int32_t)(count - (size_t)bound);
            c.n_short = (int32_t)few;
            counts_out[q] = c;
        } else if (count) {
            if (int e = d2h(h, idx_out + first * 4, tab[(size_t)q].idx_out, count * 4 * sizeof(int))) return e;
            if (int e = d2h(h, w_out + first * 4, tab[(size_t)q].w_out, count * 4 * sizeof(float))) return e;
            first += count;
        }
    }
    return SF_OK;
}

extern "C" {

int sfd_version(void) { return SFD_VERSION; }
size_t sfd_params_bytes(void) { return sizeof(sfd_params); }
size_t sfd_counts_bytes(void) { return sizeof(sfd_counts); }
size_t sfd_info_bytes(void) { return sizeof(sfd_info); }
size_t sfd_constraint_bytes(void) { return sizeof(sfd_constraint); }
size_t sfd_solve_params_bytes(void) { return sizeof(sfd_solve_params); }
size_t sfd_report_bytes(void) { return sizeof(sfd_report); }

int sfd_default_params(sfd_params *p) {
    if (!p) return fail(SF_ERR_ARG, "sfd_default_params: null");
    *p = sfd_params{INFINITY, {0, 0, 0, 0, 0, 0, 0}};
    return SF_OK;
}

int sfd_default_solve_params(sfd_solve_params *p) {
    if (!p) return fail(SF_ERR_ARG, "sfd_default_solve_params: null");
    *p = sfd_solve_params{INFINITY, 1.0f, 1e-6f, 8, {0, 0, 0, 0}};
    return SF_OK;
}

int sfd_check_params(const sfd_params *p) { return check_params(p); }
int sfd_check_solve_params(const sfd_solve_params *p) { return check_solve_params(p); }

int sfd_graph_create(sf_handle *h, int max_nodes, sfd_graph **out) {
    if (!h || !out) return fail(SF_ERR_ARG, "sfd_graph_create: null argument");
    if (int e = check_live_handle("sfd_graph_create", h)) return e;
    if (max_nodes < 1 || max_nodes > SFD_MAX_NODES) return fail(SF_ERR_ARG, "sfd_graph_create: max_nodes lies in 1..1024");
    sfd_graph *g = new sfd_graph;
    g->h = h;
    g->max_nodes = max_nodes;
    h->parts.enter(g);
    *out = g;
    return SF_OK;
}

void sfd_graph_destroy(sfd_graph *g) {
    if (!g) return;
    part_destroy(g);
    delete g;
}

int sfd_graph_info(const sfd_graph *g, sfd_info *info) {
    if (int e = check_graph("sfd_graph_info", g)) return e;
    if (!info) return fail(SF_ERR_ARG, "sfd_graph_info: null");
    *info = sfd_info{g->max_nodes, g->G, {0, 0}};
    return SF_OK;
}

int sfd_graph_set(sfd_graph *g, int G, const float *pos, const float *times, const float *M) {
    if (int e = check_graph("sfd_graph_set", g)) return e;
    if (G < 0 || G > g->max_nodes) return fail(SF_ERR_ARG, "sfd_graph_set: G lies in 0..max_nodes");
    if (G > 0 && (!pos || !times)) return fail(SF_ERR_ARG, "sfd_graph_set: null argument");
    if (M && !finite_all(M, 12 * G)) return fail(SF_ERR_ARG, "sfd_graph_set: NaN or inf in M");
    float *t = g->blk.resized<float>((size_t)G * 16);  // (host memory only: the next call that uses the graph sends it)
    for (int j = 0; j < G; j++) {
        for (int k = 0; k < 3; k++) t[4 * j + k] = pos[3 * j + k];
        t[4 * j + 3] = times[j];
        for (int k = 0; k < 12; k++) t[4 * (size_t)G + 12 * (size_t)j + k] = M ? M[12 * (size_t)j + k] : (k % 5 == 0 ? 1.f : 0.f);
    }
    g->G = G;
    return SF_OK;
}

int sfd_graph_get(const sfd_graph *g, float *pos, float *times, float *M) {
    if (int e = check_graph("sfd_graph_get", g)) return e;
    const int G = g->G;
    const float *t = (const float *)g->blk.host[0].data();
    for (int j = 0; j < G; j++) {
        for (int k = 0; k < 3; k++)
            if (pos) pos[3 * j + k] = t[4 * j + k];
        if (times) times[j] = t[4 * j + 3];
    }
    if (M && G) std::memcpy(M, t + 4 * (size_t)G, (size_t)G * 12 * sizeof(float));
    return SF_OK;
}

int sfd_sample_nodes(sf_map *map, float spacing, int max_nodes, float *pos_out, float *times_out, int *count_out) {
    if (!map || !pos_out || !times_out || !count_out) return fail(SF_ERR_ARG, "sfd_sample_nodes: null argument");
    if (max_nodes < 1 || max_nodes > SFD_MAX_NODES) return fail(SF_ERR_ARG, "sfd_sample_nodes: max_nodes lies in 1..1024");
    sfj_params p;
    if (int e = sfj_default_params(&p)) return e;
    p.cell = spacing;
    if (int e = sfj_check_params(&p)) return e;
    std::vector<float> kept((size_t)max_nodes * 12);
    sfj_counts c{};
    c.n_out = -1;
    const int code = sfj_thin_extract(map, &p, kept.data(), max_nodes, &c);
    if (code != SF_OK) {
        if (code == SF_ERR_ARG && c.n_out > max_nodes) {  // (the thinning's answer to too little room, with its count)
            *count_out = c.n_out;
            return fail(SF_ERR_STATE, "sfd_sample_nodes: " + std::to_string(c.n_out) + " nodes at this spacing, room for " + std::to_string(max_nodes));
        }
        return code;
    }
    for (int j = 0; j < c.n_out; j++) {
        for (int k = 0; k < 3; k++) pos_out[3 * j + k] = kept[12 * (size_t)j + k];
        times_out[j] = kept[12 * (size_t)j + 6];
    }
    *count_out = c.n_out;
    return SF_OK;
}

int sfd_bind_point(int G, const float *pos, const float *times, float time_window, const float p[3], float tau, int32_t idx_out[4], float w_out[4]) {
    if (int e = check_arrays("sfd_bind_point", G, SFD_MAX_NODES, pos, times, nullptr, false, time_window)) return e;
    if (!p || !idx_out || !w_out) return fail(SF_ERR_ARG, "sfd_bind_point: null argument");
    int idx[4];
    const int m = sfd_bind_core(G, pos, times, time_window, p, tau, -1, idx, w_out);
    for (int k = 0; k < 4; k++) idx_out[k] = idx[k];
    return m;
}

int sfd_deform_surfel(int G, const float *pos, const float *times, const float *M, float time_window, const float s[12], float out[12]) {
    if (int e = check_arrays("sfd_deform_surfel", G, SFD_MAX_NODES, pos, times, M, true, time_window)) return e;
    if (!s || !out) return fail(SF_ERR_ARG, "sfd_deform_surfel: null argument");
    float o[12];
    std::memcpy(o, s, sizeof(o));
    const int m = sfd_deform_surfel_core(G, pos, times, M, time_window, s, o);
    std::memcpy(out, o, sizeof(o));
    return m;
}

int sfd_edges(int G, const float *pos, const float *times, float time_window, int32_t *edges_out) {
    if (int e = check_arrays("sfd_edges", G, SFD_MAX_NODES, pos, times, nullptr, false, time_window)) return e;
    if (!edges_out) return fail(SF_ERR_ARG, "sfd_edges: null argument");
    for (int j = 0; j < G; j++) {
        int e4[4];
        sfd_edges_core(G, pos, times, time_window, j, e4);
        for (int k = 0; k < 4; k++) edges_out[4 * (size_t)j + k] = e4[k];
    }
    return SF_OK;
}

int sfd_deform_poses(int G, const float *pos, const float *times, const float *M, float time_window, int n, const float *poses, const float *taus,
                     float *poses_out) {
    if (int e = check_arrays("sfd_deform_poses", G, SFD_MAX_NODES, pos, times, M, true, time_window)) return e;
    if (n < 0 || (n && (!poses || !taus || !poses_out))) return fail(SF_ERR_ARG, "sfd_deform_poses: bad argument");
    for (int q = 0; q < n; q++)
        if (!finite_all(poses + 16 * (size_t)q, 16)) return fail(SF_ERR_ARG, "sfd_deform_poses: NaN or inf in a pose");
    for (int q = 0; q < n; q++) sfd_deform_pose_core(G, pos, times, M, time_window, poses + 16 * (size_t)q, taus[q], poses_out + 16 * (size_t)q);
    return SF_OK;
}

int sfd_bind_maps(sf_handle *h, int n, sf_map *const *maps, sfd_graph *const *graphs, const sfd_params *params, int32_t *idx_out, float *w_out) {
    return run("sfd_bind_maps", false, h, n, maps, graphs, params, idx_out, w_out, nullptr);
}

int sfd_apply_maps(sf_handle *h, int n, sf_map *const *maps, sfd_graph *const *graphs, const sfd_params *params, sfd_counts *counts_out) {
    return run("sfd_apply_maps", true, h, n, maps, graphs, params, nullptr, nullptr, counts_out);
}

int sfd_solve(int G, const float *pos, const float *times, int C, const sfd_constraint *constraints, const sfd_solve_params *sp, float *M, sfd_report *report_out) {
    if (int e = check_solve_params(sp)) return e;
    if (int e = check_arrays("sfd_solve", G, SFD_SOLVE_MAX_NODES, pos, times, M, true, sp->time_window)) return e;
    if (C < 0 || (C && !constraints) || !report_out) return fail(SF_ERR_ARG, "sfd_solve: bad argument");
    for (int c = 0; c < C; c++) {
        if (!finite_all(constraints[c].src, 8)) return fail(SF_ERR_ARG, "sfd_solve: NaN or inf in a constraint");
        if (constraints[c].weight < 0.f) return fail(SF_ERR_ARG, "sfd_solve: a negative weight");
    }
    sfd_report r{};
    r.status = sfd_solve_core(G, pos, times, C, (const SfdConstraint *)constraints, sp->time_window, sp->w_reg, sp->damping, sp->iterations, M, &r.iterations_done,
                              &r.n_bound, r.energy);
    r.n_unbound = C - r.n_bound;
    *report_out = r;
    return SF_OK;
}

}  // extern "C"
