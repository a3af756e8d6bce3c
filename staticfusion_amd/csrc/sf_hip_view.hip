// sf_hip_view.hip — libsf_hip.so, the interface of include/sf_view.h (symbols sfv_*): surfel buffers drawn from any pose with
// any pinhole intrinsics into depth, colour and index images (kernels: sf_view.h). A render only reads its maps. Everything
// it writes lies in the call block sf_handle::view (sf_call_block.h: layout, growth and lifetime): argument tables, one ray
// table per distinct (rows, cols, cx, cy, fx, fy) of the call, per view a key image, a large-sprite list and -- for the
// host-pointer calls -- the images before they are copied out. It uses no scratch of a map, no key image or density flag of
// the prediction, no image of a stream and not the handle's shared argument table.
#include "../../include/sf_view.h"
#include "sf_host.h"
#include "sf_view.h"

#define SFV_VERSION 1
static_assert(sizeof(sfv_view) == 112, "include/sf_view.h: sfv_view is 112 bytes");

static int check_view(const sfv_view *v) {
    if (!v) return fail(SF_ERR_ARG, "sfv: null view");
    if (!finite_all(v->pose, 16) || !finite_all(&v->cx, 4) || !std::isfinite(v->min_confidence) || !std::isfinite(v->max_depth))
        return fail(SF_ERR_ARG, "sfv: NaN or inf in a view");
    if (v->rows < 1 || v->rows > 4096 || v->cols < 1 || v->cols > 4096) return fail(SF_ERR_ARG, "sfv: rows and cols of a view lie in 1..4096");
    if (v->fx == 0.f || v->fy == 0.f) return fail(SF_ERR_ARG, "sfv: fx or fy of a view is 0");
    if (!(v->max_depth > 0.4f)) return fail(SF_ERR_ARG, "sfv: max_depth of a view must exceed 0.4");
    if (v->shade != SFV_SHADE_COLOUR && v->shade != SFV_SHADE_NORMAL) return fail(SF_ERR_ARG, "sfv: unknown shade");
    return SF_OK;
}

// ---- the drawing stage (declared in sf_host.h: sf_hip_score.hip draws into a block of its own with it)
void sfv_plan(ViewPlan &p, int n, const ViewJob *jobs, const sfv_view *views, int upload_count) {
    p.n = n;
    p.ray_of.assign((size_t)n, 0);
    p.ray_first.clear();
    for (int q = 0; q < n; q++) {  // distinct ray tables
        const sfv_view &v = views[q];
        int r = 0;
        for (; r < (int)p.ray_first.size(); r++) {
            const sfv_view &w = views[p.ray_first[(size_t)r]];
            if (w.rows == v.rows && w.cols == v.cols && w.cx == v.cx && w.cy == v.cy && w.fx == v.fx && w.fy == v.fy) break;
        }
        if (r == (int)p.ray_first.size()) p.ray_first.push_back(q);
        p.ray_of[(size_t)q] = r;
    }
    p.off = 0;
    p.o_tab = p.take((size_t)n * sizeof(ViewArgs));
    p.o_rtab = p.take(p.ray_first.size() * sizeof(ViewRayArgs));
    p.o_counters = p.take((size_t)n * sizeof(int));
    p.o_upload = p.take((size_t)upload_count * 12 * sizeof(float));
    p.o_rays.resize(p.ray_first.size());
    p.o_keys.resize((size_t)n);
    p.o_list.resize((size_t)n);
    for (size_t r = 0; r < p.ray_first.size(); r++)
        p.o_rays[r] = p.take((size_t)views[p.ray_first[r]].rows * views[p.ray_first[r]].cols * sizeof(vfloat4));
    for (int q = 0; q < n; q++) {
        p.o_keys[(size_t)q] = p.take((size_t)views[q].rows * views[q].cols * 8);
        p.o_list[(size_t)q] = p.take((size_t)jobs[q].count * sizeof(int));
    }
}

int sfv_draw_keys(sf_handle *h, const ViewPlan &p, const ViewJob *jobs, const sfv_view *views, const ViewOut *outs, SfCallBlock &blk,
                  const float *upload, int upload_count) {
    const int n = p.n;
    unsigned char *base = blk.dev;
    unsigned char *tab_host = blk.resized<unsigned char>(p.o_counters);  // both tables, as they lie in the block
    ViewArgs *tab = (ViewArgs *)(tab_host + p.o_tab);
    ViewRayArgs *rtab = (ViewRayArgs *)(tab_host + p.o_rtab);
    int max_count = 0;
    size_t max_px = 0, max_ray_px = 0;
    for (size_t r = 0; r < p.ray_first.size(); r++) {
        const sfv_view &v = views[p.ray_first[r]];
        rtab[r] = ViewRayArgs{(vfloat4 *)(base + p.o_rays[r]), v.rows, v.cols, v.cx, v.cy, v.fx, v.fy};
        max_ray_px = std::max(max_ray_px, (size_t)v.rows * v.cols);
    }
    for (int q = 0; q < n; q++) {
        const sfv_view &v = views[q];
        ViewArgs &a = tab[q];
        a.surfels = jobs[q].d_surfels ? jobs[q].d_surfels : (const float *)(base + p.o_upload);
        a.count = jobs[q].count;
        invert_pose(v.pose, a.t_inv);  // the prediction's t_inv = pose.inverse()
        a.cx = v.cx; a.cy = v.cy; a.fx = v.fx; a.fy = v.fy;
        a.max_depth = v.max_depth;
        a.min_confidence = v.min_confidence;
        a.tick = float(jobs[q].tick);
        a.max_age = float(v.max_age);
        a.use_age = v.max_age >= 0;
        a.shade = v.shade;
        a.rows = v.rows; a.cols = v.cols;
        a.keys = (unsigned long long *)(base + p.o_keys[(size_t)q]);
        a.rays = (const vfloat4 *)(base + p.o_rays[(size_t)p.ray_of[(size_t)q]]);
        a.large_count = (int *)(base + p.o_counters) + q;
        a.large_list = (int *)(base + p.o_list[(size_t)q]);
        a.depth = outs ? (float *)outs[q].depth : nullptr;
        a.rgb = outs ? (uint8_t *)outs[q].rgb : nullptr;
        a.index = outs ? (int *)outs[q].index : nullptr;
        max_count = std::max(max_count, a.count);
        max_px = std::max(max_px, (size_t)v.rows * v.cols);
    }
    if (int e = blk.upload(0, tab_host, p.o_counters, h->stream)) return e;
    if (upload_count) HIP_TRY(hipMemcpyAsync(base + p.o_upload, upload, (size_t)upload_count * 12 * sizeof(float), hipMemcpyHostToDevice, h->stream));
    const ViewArgs *d_tab = (const ViewArgs *)(base + p.o_tab);
    const unsigned nv = (unsigned)n;
    hipLaunchKernelGGL(sfv_rays_kernel, dim3((unsigned)((max_ray_px + 255) / 256), (unsigned)p.ray_first.size()), dim3(256), 0, h->stream,
                       (const ViewRayArgs *)(base + p.o_rtab));
    hipLaunchKernelGGL(sfv_clear_kernel, dim3((unsigned)((max_px + 255) / 256), nv), dim3(256), 0, h->stream, d_tab);
    if (max_count) {
        hipLaunchKernelGGL(sfv_splat_kernel, dim3((unsigned)((max_count + SFV_SPLAT_NT - 1) / SFV_SPLAT_NT), nv), dim3(SFV_SPLAT_NT), 0, h->stream, d_tab);
        const int per_block = SFV_LARGE_NT / 64;
        hipLaunchKernelGGL(sfv_large_kernel, dim3((unsigned)std::min(SFV_LARGE_BLOCKS, (max_count + per_block - 1) / per_block), nv), dim3(SFV_LARGE_NT), 0,
                           h->stream, d_tab);
    }
    HIP_TRY(hipGetLastError());
    return SF_OK;
}

// n checked views: the drawing stage into the handle's view scratch, then resolve and -- for host outputs -- the copies
static int render(sf_handle *h, int n, const ViewJob *jobs, const sfv_view *views, const ViewOut *outs, bool device_out, const float *upload,
                  int upload_count) {
    HIP_TRY(hipSetDevice(h->device));
    ViewPlan p;
    sfv_plan(p, n, jobs, views, upload_count);
    std::vector<size_t> o_depth((size_t)n), o_rgb((size_t)n), o_index((size_t)n);
    int max_tiles = 0;
    for (int q = 0; q < n; q++) {
        const size_t px = (size_t)views[q].rows * views[q].cols;
        if (!device_out) {
            if (outs[q].depth) o_depth[(size_t)q] = p.take(px * 4);
            if (outs[q].rgb) o_rgb[(size_t)q] = p.take(px * 3);
            if (outs[q].index) o_index[(size_t)q] = p.take(px * 4);
        }
        max_tiles = std::max(max_tiles, ((views[q].rows + SFV_T - 1) / SFV_T) * ((views[q].cols + SFV_T - 1) / SFV_T));
    }
    if (int e = h->view.grow(h->own, p.off, h->stream)) return e;
    unsigned char *base = h->view.dev;
    std::vector<ViewOut> staged;
    if (!device_out) {
        staged.resize((size_t)n);
        for (int q = 0; q < n; q++)
            staged[(size_t)q] = ViewOut{outs[q].depth ? base + o_depth[(size_t)q] : nullptr, outs[q].rgb ? base + o_rgb[(size_t)q] : nullptr,
                                        outs[q].index ? base + o_index[(size_t)q] : nullptr};
    }
    if (int e = sfv_draw_keys(h, p, jobs, views, device_out ? outs : staged.data(), h->view, upload, upload_count)) return e;
    hipLaunchKernelGGL(sfv_resolve_kernel, dim3((unsigned)max_tiles, (unsigned)n), dim3(256), 0, h->stream, (const ViewArgs *)(base + p.o_tab));
    HIP_TRY(hipGetLastError());
    h->view_counters_off = p.o_counters;
    h->view_last_n = n;
    if (device_out) return SF_OK;
    HIP_TRY(hipStreamSynchronize(h->stream));  // the images are in the block, and an uploaded host buffer is free again
    for (int q = 0; q < n; q++) {
        const size_t px = (size_t)views[q].rows * views[q].cols;
        if (outs[q].depth) HIP_TRY(hipMemcpy(outs[q].depth, base + o_depth[(size_t)q], px * 4, hipMemcpyDeviceToHost));
        if (outs[q].rgb) HIP_TRY(hipMemcpy(outs[q].rgb, base + o_rgb[(size_t)q], px * 3, hipMemcpyDeviceToHost));
        if (outs[q].index) HIP_TRY(hipMemcpy(outs[q].index, base + o_index[(size_t)q], px * 4, hipMemcpyDeviceToHost));
    }
    return SF_OK;
}

static int render_maps(const char *what, sf_handle *h, int n, sf_map *const *maps, const sfv_view *views, void *const *depth_out, void *const *rgb_out,
                       void *const *index_out, bool device_out) {
    if (!h || n < 0 || (n && (!maps || !views))) return fail(SF_ERR_ARG, std::string(what) + ": bad argument");
    if (n == 0) return SF_OK;
    if (int e = check_batch(what, n, "views")) return e;
    std::vector<ViewJob> jobs((size_t)n);
    std::vector<ViewOut> outs((size_t)n);
    for (int q = 0; q < n; q++) {
        const sf_map *m = maps[q];
        if (int e = check_map(what, h, m)) return e;
        if (int e = check_view(views + q)) return e;
        jobs[(size_t)q] = ViewJob{m->buf[0], m->count, m->tick};
        outs[(size_t)q] = ViewOut{depth_out ? depth_out[q] : nullptr, rgb_out ? rgb_out[q] : nullptr, index_out ? index_out[q] : nullptr};
    }
    return render(h, n, jobs.data(), views, outs.data(), device_out, nullptr, 0);
}

extern "C" {

int sfv_version(void) { return SFV_VERSION; }
size_t sfv_view_bytes(void) { return sizeof(sfv_view); }
int sfv_check_view(const sfv_view *v) { return check_view(v); }

int sfv_default_view(const sf_handle *h, sf_map *m, sfv_view *v) {
    if (!h || !v) return fail(SF_ERR_ARG, "sfv_default_view: null");
    if (m)  // (a null map is allowed: the identity pose)
        if (int e = check_map("sfv_default_view", h, m)) return e;
    sf_model_params p;
    if (int e = sf_default_model_params(h, &p)) return e;
    for (int k = 0; k < 16; k++) v->pose[k] = m ? m->pose[k] : ((k % 5 == 0) ? 1.f : 0.f);
    v->cx = p.cx; v->cy = p.cy; v->fx = p.fx; v->fy = p.fy;
    v->rows = h->k.rows; v->cols = h->k.cols;
    v->min_confidence = 0.25f;
    v->max_depth = 20.0f;
    v->max_age = -1;
    v->shade = SFV_SHADE_COLOUR;
    return SF_OK;
}

int sfv_render_maps(sf_handle *h, int n, sf_map *const *maps, const sfv_view *views, float *const *depth_out, uint8_t *const *rgb_out,
                    int32_t *const *index_out) {
    return render_maps("sfv_render_maps", h, n, maps, views, (void *const *)depth_out, (void *const *)rgb_out, (void *const *)index_out, false);
}

int sfv_render_maps_device(sf_handle *h, int n, sf_map *const *maps, const sfv_view *views, void *const *depth_out, void *const *rgb_out,
                           void *const *index_out) {
    return render_maps("sfv_render_maps_device", h, n, maps, views, depth_out, rgb_out, index_out, true);
}

int sfv_render_surfels(sf_handle *h, const float *surfels, int count, int tick, const sfv_view *view, float *depth, uint8_t *rgb, int32_t *index) {
    if (!h || count < 0 || (!surfels && count > 0)) return fail(SF_ERR_ARG, "sfv_render_surfels: bad argument");
    if (int e = check_view(view)) return e;
    const ViewJob job{nullptr, count, tick};
    const ViewOut out{depth, rgb, index};
    return render(h, 1, &job, view, &out, false, surfels, count);
}

int sfv_last_large_sprites(sf_handle *h, int n, int32_t *counts) {
    if (!h || !counts || n < 0) return fail(SF_ERR_ARG, "sfv_last_large_sprites: bad argument");
    if (n != h->view_last_n || !h->view.dev) return fail(SF_ERR_STATE, "sfv_last_large_sprites: n is not the n of the handle's last render call");
    if (n == 0) return SF_OK;
    return d2h(h, counts, h->view.dev + h->view_counters_off, (size_t)n * sizeof(int32_t));
}

}  // extern "C"
