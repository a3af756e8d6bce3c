// sf_host.h — what the host-side translation units of libsf_hip.so share: the handle, the error helpers, device
// allocation, the refusals that every companion interface states the same way, and the few functions one part calls in
// another. Nothing here is exported (include/sf.h is the ABI).
//   sf_resources.h     the owner of every device block, pinned block, event and stream (SfOwner), the one growth rule
//                      (SfOwner::grow, here dev_grow) and the ring of per-call tables (SfRing); host only, no kernel
//   sf_call_block.h    the per-call block of a companion interface: its layout rule (SfPlan), the block with the host copies
//                      of its tables (SfCallBlock) and the rules of their lifetime; host only, no kernel
//   sf_parts.h         what is created from a handle and may outlive it (maps, keyframe databases, trackers, deformation
//                      graphs, closure builders, carvers, registrars): their base (SfPart), the handle's list of them (SfParts) and the rules of
//                      their lifetime; host only, no kernel
//   sf_hip.hip         handle lifetime and the list of live handles, parameters, the builds of the frame kernel, launch()
//   sf_hip_solver.hip  images in, frames (one or several per launch), results and debug planes out, measurement support
//   sf_hip_input.hip   the input stage: loader decimation / RGB -> intensity, bilateral depth filter (sf_input.h)
//   sf_hip_model.hip   frame-to-model prediction and the surfel map without OpenGL (sf_predict.h, sf_fusion.h); the map
//                      check and the table upload of every part that takes maps (check_map, upload_table)
//   sf_hip_migrate.hip single streams between handles, to and from host memory, back to constructor state (sf_migrate.h;
//                      its interface is include/sf_migrate.h, symbols sfm_*)
//   sf_hip_map_window.hip  bounded maps: count, cull, extract, page out, append (sf_map_window.h, sf_window_args.h; its
//                      interface is include/sf_map_window.h, symbols sfw_*); the one compiled copy of the scan and the
//                      ordered write, which the join and the body maps launch through sfw_launch_scan / sfw_launch_write
//   sf_hip_view.hip    maps drawn from any view: depth, colour and index images (sf_view.h; its interface is
//                      include/sf_view.h, symbols sfv_*)
//   sf_hip_score.hip   poses scored against maps: frame-to-map agreement counts (sf_score.h; its interface is
//                      include/sf_score.h, symbols sfs_*)
//   sf_hip_keyframes.hip  place recognition: fern-coded keyframes that propose poses (sf_keyframes.h; its interface is
//                      include/sf_keyframes.h, symbols sfk_*)
//   sf_hip_regions.hip moving regions: connected components of the dynamic pixels, numbered, with statistics
//                      (sf_regions.h; its interface is include/sf_regions.h, symbols sfr_*)
//   sf_hip_align.hip   poses refined against maps: damped point-to-plane steps with integer normal equations
//                      (sf_align.h; its interface is include/sf_align.h, symbols sfa_*). What it shares with the region
//                      motion and the registration: the quantised system (sf_p2p_system.h), the step (sf_align_step.h), and
//                      an entry's state, the workgroup's reduction and the step's bookkeeping (sf_p2p_device.h)
//   sf_hip_join.hip    maps joined and thinned on a voxel grid: merge, decimate (sf_join.h, sf_join_key.h; its interface
//                      is include/sf_join.h, symbols sfj_*). The voxel table and its insert kernel, which the registration
//                      uses too: sf_voxel_table.h
//   sf_hip_tracks.hip  region tracks: the moving regions followed from frame to frame, with a metric box (sf_tracks.h,
//                      sf_track_assign.h; its interface is include/sf_tracks.h, symbols sft_*)
//   sf_hip_bodies.hip  region motion: the rigid motion of every moving region between two frames (sf_bodies.h,
//                      sf_body_world.h; its interface is include/sf_bodies.h, symbols sfb_*)
//   sf_hip_body_maps.hip  body maps: every moving region fused into a surfel map of its own (sf_body_maps.h,
//                      sf_body_map_rules.h; its interface is include/sf_body_maps.h, symbols sfp_*)
//   sf_hip_deform.hip  deformation graphs: maps bent by the nodes of a graph, and the solver for their transforms
//                      (sf_deform.h, sf_deform_rules.h, sf_deform_solve.h; its interface is include/sf_deform.h, symbols sfd_*)
//   sf_hip_closure.hip loop closures: constraints from two drawings of a place (sf_closure.h, sf_closure_rules.h; its
//                      interface is include/sf_closure.h, symbols sfc_*)
//   sf_hip_carve.hip   carving: surfels that later frames saw through leave their maps (sf_carve.h, sf_carve_rules.h; its
//                      interface is include/sf_carve.h, symbols sfe_*)
//   sf_hip_register.hip  registration: surfel maps aligned with each other on the voxel tables of their destinations
//                      (sf_register.h, sf_register_rules.h, sf_voxel_table.h; its interface is include/sf_register.h, symbols sfg_*)
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "sf_cluster.h"
#include "sf_device_common.h"
#include "sf_parts.h"  // SfPart, SfParts; sf_call_block.h: SfPlan, SfCallBlock; sf_resources.h: SF_INTERNAL, sf_fail, SfOwner, SfRing

// the two builds of the frame kernels (sf_frame_kernels.hip, -DSF_NT=256 / -DSF_NT=1024)
struct FrameVariant {
    int id;  // SF_VARIANT_*
    const char *name;
    void (*geometry)(int *threads, int *blocks_per_cu);
    void (*launch_frame)(int grid, hipStream_t st, const KArgs *ka, const FrameLaunch *fl);
    void (*launch_irls_pass)(int grid, hipStream_t st, const KArgs *ka, int which, int variant, int reps, int slices, int window_px);
    void (*launch_debug_rows)(int grid, hipStream_t st, const KArgs *ka, int b, float *out);
};

struct sf_handle {
    KArgs k{};
    int device = 0;
    int max_blocks = 0;
    int wg_per_cu = 0;
    int *d_order = nullptr;   // KArgs::order storage (more streams than resident workgroups: a launch has a tail)
    int max_blocks_o5 = 0;  // throughput build: resident workgroups of the 5-per-CU kernel (0: not used)
    const FrameVariant *fv = nullptr;  // set by sf_create_ex
    SfParts parts;  // what was created from this handle and lives: maps, keyframe databases, trackers, graphs, builders, carvers, registrars (sf_parts.h)
    bool reforder = false;  // the library's frame kernels are the reference-order build (sf_reforder.h)
    int cluster_grid = 0;  // SF_VARIANT_CLUSTER: blocks per launch (8 XCDs x streams per XCD x workgroups per stream)
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, evk0 = nullptr, evk1 = nullptr;
    bool solver_timed = false;
    KArgs *d_args = nullptr;  // device copy of k (geometry, parameters, buffer table)
    bool args_dirty = true;
    SfOwner own;  // every device block, pinned block, event and stream of the handle (sf_resources.h): sf_destroy releases it
    // input stage (sf_input.h), allocated by the first sf_load_frame*
    float depth_cutoff = 4.5f;  // FrontEnd.cpp:168
    bool have_frame = false;
    uint16_t *in_depth_mm = nullptr, *in_filtered_mm = nullptr;
    float *in_depth_metric = nullptr;
    uint8_t *in_color = nullptr;
    uint8_t *stage_color = nullptr;  // one full-resolution frame, for the host-pointer variant
    uint16_t *stage_depth = nullptr;
    size_t stage_color_cap = 0, stage_depth_cap = 0;  // capacities in elements (dev_grow)
    // model prediction (sf_predict.h), allocated by the first sf_predict_from_model
    unsigned long long *pr_keys = nullptr;  // per batched map: low and high key image (2 x n0)
    int *pr_dense = nullptr;                // per batched map: 2 ints (density sum; init-model counts)
    size_t pr_keys_cap = 0, pr_dense_cap = 0;  // capacities of the two blocks above in elements (dev_grow)
    bool pr_rendered = false;
    std::vector<int> pr_job_of_stream;      // per stream: index of the job of the last predict batch that rendered into it, or -1
    vfloat4 *pr_rays = nullptr;             // view ray per pixel for the intrinsics below (sf_predict_rays_kernel)
    float pr_rays_for[4] = {0.f, 0.f, 0.f, 0.f};
    float *pr_surfels = nullptr;
    size_t pr_floats = 0;                   // capacity of pr_surfels in floats (12 per surfel)
    // argument tables of the batched map kernels (sf_predict.h, sf_fusion.h): device block + the host copy it is filled from
    unsigned char *tab_dev = nullptr;
    size_t tab_bytes = 0;
    std::vector<unsigned char> tab_host;
    int *res_dev = nullptr;                 // per batched map: 8 ints of results
    size_t res_ints = 0;                    // capacity of res_dev in ints
    // overlapped host -> HBM upload of the next frames (sf_upload_current_async): copy stream, staging, event
    hipStream_t copy_stream = nullptr;
    hipEvent_t copy_done = nullptr, compute_done = nullptr;
    float *up_depth = nullptr, *up_inten = nullptr;
    bool upload_pending = false;
    // sf_advance_sequences_device: per-stream frame numbers, a ring of device + pinned host slots so that calls queue up
    // behind running frame kernels without a host synchronisation (a slot is reused only after its copy has executed).
    // All eight slots are made by the first call: no later call allocates.
    SfRing<8, true> seq_ring;
    // multi-frame launches (sf_process_frames / sf_process_sequence_frames_device)
    int *d_frame_done = nullptr;     // [batch]
    int *d_multi_index = nullptr;    // [frames][batch]
    int *h_multi_index = nullptr;    // pinned staging of the same size
    float *d_traj = nullptr;         // [frames][batch][16]
    size_t d_multi_cap = 0, h_multi_cap = 0, traj_cap = 0;  // capacities of the three in elements (dev_grow)
    int solver_timed_frames = 1;     // frames of the launch evk0 / evk1 bracket
    // stream migration (sf_hip_migrate.hip): the per-call segment tables, a ring of device + pinned host slots like the one of
    // sf_advance_sequences_device (a call queues up behind running kernels; a slot is reused after its kernel has executed)
    // whose slots are made one by one as calls first reach them, the event the two handles of a copy order their HIP streams
    // with, and the staging block of export / import
    SfRing<4, false> mig_ring;
    hipEvent_t mig_ev = nullptr;
    uint8_t *mig_stage = nullptr;
    size_t mig_stage_bytes = 0;
    // The companion interfaces: per part one call block (sf_call_block.h: device memory grown when a call needs more, the host
    // copies its tables are filled from, and the rules of their lifetime). What lies in each is its file's business.
    SfCallBlock view;       // sf_hip_view.hip: free-view rendering
    size_t view_counters_off = 0;  // where the per-view list counters of the last render call lie in `view`, and its n
    int view_last_n = 0;
    SfCallBlock score;      // sf_hip_score.hip: the drawing layout (ViewPlan), then the score table, records, frames
    SfCallBlock regions;    // sf_hip_regions.hip
    SfCallBlock align;      // sf_hip_align.hip: the drawing layout, then the entry table with the states, images, systems
    SfCallBlock join;       // sf_hip_join.hip
    SfCallBlock bodies;     // sf_hip_bodies.hip: host copy 0 the entry table, host copy 1 the pair table
    SfCallBlock body_maps;  // sf_hip_body_maps.hip
};

// the surfel map (sf_hip_model.hip creates, fuses and releases it; sf_hip_map_window.hip partitions it)
struct SF_INTERNAL sf_map : SfPart {  // (own: the map's device blocks, not zero-filled)
    int capacity = 0;
    float *buf[2] = {nullptr, nullptr};  // the model lives in buf[0] between calls; buf[1] holds the merged model inside a fuse
    int count = 0, tick = 1;
    float pose[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    int stats[4] = {0, 0, 0, 0};
    unsigned long long *keys = nullptr, *occ = nullptr;
    unsigned *winner = nullptr, *meta = nullptr, *index_export = nullptr;
    float *rec = nullptr;
    unsigned char *flags = nullptr;
    int *block_counts = nullptr;
    bool have_index = false;
    int epoch = 0;  // index images rendered since the key image was last filled with ones; tag = 255 - epoch
    void shelled() override {
        buf[0] = buf[1] = rec = nullptr;
        keys = occ = nullptr;
        winner = meta = index_export = nullptr;
        flags = nullptr;
        block_counts = nullptr;
    }
};

// Constructor state of a stream (reference FrontEnd.cpp:79-81,110,152-154), as the 32-bit word at byte offset `off` of its
// StreamState: T_odometry and the pose ring are identity, b_segm 0.5, conn[l] = 1 << l, perClusterAverageResidual NaN, kb the
// handle's, everything else zero. sf_create_ex fills the whole struct from it; sfm_reset_streams the members that travel.
__host__ __device__ static inline uint32_t sf_ctor_state_word(size_t off, float kb) {
    const uint32_t one = 0x3f800000u, half = 0x3f000000u, quiet_nan = 0x7fc00000u;
    const size_t w = off / 4;
#define SF_IN(member) (off >= offsetof(StreamState, member) && off < offsetof(StreamState, member) + sizeof(StreamState::member))
    if (SF_IN(T)) return ((w - offsetof(StreamState, T) / 4) % 5 == 0) ? one : 0u;
    if (SF_IN(hist_T)) return (((w - offsetof(StreamState, hist_T) / 4) % 16) % 5 == 0) ? one : 0u;
    if (SF_IN(b_segm)) return half;
    if (SF_IN(conn)) return 1u << (w - offsetof(StreamState, conn) / 4);
    if (SF_IN(cluster_res)) return quiet_nan;
    if (SF_IN(kb)) {
        union { float f; uint32_t u; } v;
        v.f = kb;
        return v.u;
    }
#undef SF_IN
    return 0u;
}

#define fail sf_fail  // (sf_resources.h)
#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return fail(SF_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));             \
    } while (0)

// a zero-filled device block of the handle, and the growth rule on the handle's stream (SfOwner: sf_resources.h)
template <class T>
static int dev_alloc(sf_handle *h, T **p, size_t count) {
    return h->own.device(p, count);
}
template <class T>
static int dev_grow(sf_handle *h, T **p, size_t *capacity, size_t count) {
    return h->own.grow(p, capacity, count, h->stream);
}

// ---- the shared refusal list of the companion interfaces. Each takes the caller's name (or its prefix), so a refusal names
// its function; a caller makes them in the order its header promises, and a refused call has changed nothing.
enum CallForm { FORM_STREAMS, FORM_HOST, FORM_DEVICE };  // the inputs of a call: the handle's streams, host images, device images
// the batch bound: n entries, at most 65535 (grid.y); n == 0 is the caller's to answer
static inline int check_batch(const std::string &w, int n, const char *noun = "entries") {
    if (n < 0) return fail(SF_ERR_ARG, w + ": n < 0");
    if (n > 65535) return fail(SF_ERR_ARG, w + ": more than 65535 " + noun + " in one call");
    return SF_OK;
}
// the image-size rule of the calls that take frames of a size of their own
static inline int check_image_size(const std::string &w, int rows, int cols) {
    if (rows < 1 || rows > 4096 || cols < 1 || cols > 4096 || (long long)rows * cols > (1ll << 24))
        return fail(SF_ERR_ARG, w + ": rows and cols lie in 1..4096 and rows * cols <= 2^24");
    return SF_OK;
}
static inline bool finite_all(const float *p, int n) {
    for (int i = 0; i < n; i++)
        if (!std::isfinite(p[i])) return false;
    return true;
}
// sft_camera, sfb_camera, sfp_camera (one layout: their files assert it): pose[16], then cx, cy, fx, fy
template <class Camera>
static int check_camera(const char *prefix, const Camera *c) {
    if (!finite_all(c->pose, 16) || !finite_all(&c->cx, 4)) return fail(SF_ERR_ARG, std::string(prefix) + ": NaN or inf in a camera");
    if (c->fx == 0.f || c->fy == 0.f) return fail(SF_ERR_ARG, std::string(prefix) + ": fx or fy is 0");
    return SF_OK;
}
// the distinct-maps check, entry by entry: maps[q] is none of maps[0 .. q)
static inline int check_distinct(const std::string &w, sf_map *const *maps, int q, const char *twice) {
    for (int r = 0; r < q; r++)
        if (maps[r] == maps[q]) return fail(SF_ERR_ARG, w + ": " + twice);
    return SF_OK;
}
// the rule AFTER A CALL THAT CHANGES A MAP of include/sf_map_window.h: surfel indices have moved, so the index image of the
// last fuse no longer describes the map
static inline void indices_moved(sf_map *m) { m->have_index = false; }

// shared between the parts (defined in the file named)
SF_INTERNAL int launch(sf_handle *h, int mask, int im_count, int n_frames = 1, const FrameLaunch *ml = nullptr);  // sf_hip.hip
SF_INTERNAL int solve_mask(const sf_handle *h, int create_image_pyr);                                            // sf_hip.hip
SF_INTERNAL int pass_window_px(int resident_workgroups);                                                          // sf_hip.hip
SF_INTERNAL bool use_five_per_cu(const sf_handle *h);                                                           // sf_hip.hip
// The drawing stage of a batch of views, shared by the render calls and the score calls (sf_hip_view.hip). sfv_plan lays the
// tables, ray tables, key images and large-sprite lists of n checked views out from offset 0 of a block; the caller takes
// what else it needs behind them (ViewPlan::take), grows its block to ViewPlan::off bytes and hands it to sfv_draw_keys,
// which fills and uploads the tables and launches rays, clear, splat and large sprites on the handle's stream. Afterwards
// the key image of view q is complete at base + o_keys[q] and its ViewArgs at d_tab[q].
struct ViewJob {
    const float *d_surfels;  // device; null with upload != null: the uploaded copy in the block
    int count, tick;
};
struct ViewOut {
    void *depth, *rgb, *index;  // device pointers of the resolve kernel's outputs, any of them null
};
struct ViewPlan : SfPlan {
    int n = 0;
    std::vector<int> ray_of;     // per view: its ray table
    std::vector<int> ray_first;  // per ray table: the view that introduced it
    size_t o_tab = 0, o_rtab = 0, o_counters = 0, o_upload = 0;
    std::vector<size_t> o_rays, o_keys, o_list;
};
SF_INTERNAL void sfv_plan(ViewPlan &p, int n, const ViewJob *jobs, const struct sfv_view *views, int upload_count);
// (blk: the caller's block, grown to p.off bytes; the view tables are filled into its host copy 0)
SF_INTERNAL int sfv_draw_keys(sf_handle *h, const ViewPlan &p, const ViewJob *jobs, const struct sfv_view *views, const ViewOut *outs,
                              SfCallBlock &blk, const float *upload, int upload_count);
// The scan and the ordered write of sf_map_window.h for whoever has filled ballots and block counts of its own (the join, the
// body maps), on the handle's stream (sf_hip_map_window.hip: the library holds these kernels once): sfw_scan_kernel over n
// entries of a device table, sfw_write_kernel<false> over (blocks, n).
struct WindowArgs;  // sf_window_args.h
SF_INTERNAL void sfw_launch_scan(sf_handle *h, const WindowArgs *d_tab, int n);
SF_INTERNAL void sfw_launch_write(sf_handle *h, const WindowArgs *d_tab, unsigned blocks, int n);
// sf_hip.hip: the list of live handles (sf_create_ex enters a handle, sf_destroy takes it out), by which the calls that take
// a handle and no part of it refuse one that is gone
SF_INTERNAL bool handle_alive(const sf_handle *h);
static inline int check_live_handle(const std::string &where, const sf_handle *h) {
    if (!handle_alive(h)) return fail(SF_ERR_STATE, where + ": this handle has been destroyed");
    return SF_OK;
}
// ---- the parts of a handle (sf_parts.h: the rules). The two refusals every call on a part begins with: `where` is the
// caller's name, or null for the map calls whose refusals carry none; `noun` is what the part is called.
static inline int check_part(const char *where, const SfPart *p, const char *noun) {
    const std::string w = where ? std::string(where) + ": " : std::string();
    if (!p) return fail(SF_ERR_ARG, w + "null " + noun);
    if (!p->h) return fail(SF_ERR_STATE, w + "the handle this " + noun + " was created from has been destroyed");
    return SF_OK;
}
// the part goes before its handle: the handle's device, after its queued work (a shell: nothing). The caller deletes it.
static inline void part_destroy(SfPart *p) {
    sf_handle *h = p->h;
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    h->parts.leave(p);
    p->own.release_all();
}
extern "C" {  // (defined inside the extern "C" blocks of their files)
SF_INTERNAL int check_stream(const sf_handle *h, int stream);                 // sf_hip.hip
SF_INTERNAL int d2h(sf_handle *h, void *dst, const void *src, size_t bytes);  // sf_hip_solver.hip: drain the handle's stream, then copy
SF_INTERNAL int input_alloc(sf_handle *h);                                    // sf_hip_input.hip: buffers of the input stage, on first use
SF_INTERNAL void invert_pose(const float pose[16], float out[16]);            // sf_hip_model.hip: t_inv of the prediction, the fusion and the views
// sf_hip_model.hip: a map handed to `what` beside h is not null (SF_ERR_ARG), not a shell (SF_ERR_STATE) and h's own (SF_ERR_ARG)
SF_INTERNAL int check_map(const char *what, const sf_handle *h, const sf_map *m);
// sf_hip_model.hip: the table of a batched launch into h->tab_dev (grown on demand; it stays there for later launches of the call)
SF_INTERNAL int upload_table(sf_handle *h, const void *src, size_t bytes, void **dev);
SF_INTERNAL int results_scratch(sf_handle *h, size_t n_maps);                 // sf_hip_model.hip: h->res_dev holds 8 ints per batched map
}
