// sf_host.h — what the host-side translation units of libsf_hip.so share: the handle, the error helpers, device
// allocation, and the few functions one part calls in another. Nothing here is exported (include/sf.h is the ABI).
//   sf_resources.h     the owner of every device block, pinned block, event and stream (SfOwner), the one growth rule
//                      (SfOwner::grow, here dev_grow) and the ring of per-call tables (SfRing); host only, no kernel
//   sf_hip.hip         handle lifetime, parameters, the builds of the frame kernel, launch()
//   sf_hip_solver.hip  images in, frames (one or several per launch), results and debug planes out, measurement support
//   sf_hip_input.hip   the input stage: loader decimation / RGB -> intensity, bilateral depth filter (sf_input.h)
//   sf_hip_model.hip   frame-to-model prediction and the surfel map without OpenGL (sf_predict.h, sf_fusion.h); the map
//                      check and the table upload of every part that takes maps (check_map, upload_table)
//   sf_hip_migrate.hip single streams between handles, to and from host memory, back to constructor state (sf_migrate.h;
//                      its interface is include/sf_migrate.h, symbols sfm_*)
//   sf_hip_map_window.hip  bounded maps: count, cull, extract, page out, append (sf_map_window.h; its interface is
//                      include/sf_map_window.h, symbols sfw_*)
//   sf_hip_view.hip    maps drawn from any view: depth, colour and index images (sf_view.h; its interface is
//                      include/sf_view.h, symbols sfv_*)
//   sf_hip_score.hip   poses scored against maps: frame-to-map agreement counts (sf_score.h; its interface is
//                      include/sf_score.h, symbols sfs_*)
//   sf_hip_keyframes.hip  place recognition: fern-coded keyframes that propose poses (sf_keyframes.h; its interface is
//                      include/sf_keyframes.h, symbols sfk_*)
//   sf_hip_regions.hip moving regions: connected components of the dynamic pixels, numbered, with statistics
//                      (sf_regions.h; its interface is include/sf_regions.h, symbols sfr_*)
//   sf_hip_align.hip   poses refined against maps: damped point-to-plane steps with integer normal equations
//                      (sf_align.h, sf_align_step.h; its interface is include/sf_align.h, symbols sfa_*)
//   sf_hip_join.hip    maps joined and thinned on a voxel grid: merge, decimate (sf_join.h, sf_join_key.h; its interface
//                      is include/sf_join.h, symbols sfj_*)
//   sf_hip_tracks.hip  region tracks: the moving regions followed from frame to frame, with a metric box (sf_tracks.h,
//                      sf_track_assign.h; its interface is include/sf_tracks.h, symbols sft_*)
//   sf_hip_bodies.hip  region motion: the rigid motion of every moving region between two frames (sf_bodies.h,
//                      sf_body_world.h; its interface is include/sf_bodies.h, symbols sfb_*); the list of live handles
//   sf_hip_body_maps.hip  body maps: every moving region fused into a surfel map of its own (sf_body_maps.h,
//                      sf_body_map_rules.h; its interface is include/sf_body_maps.h, symbols sfp_*)
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
#include "sf_resources.h"  // SF_INTERNAL, sf_fail, SfOwner, SfRing

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
    std::vector<struct sf_map *> maps;  // live maps created from this handle: sf_destroy releases their memory and orphans them
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
    // free-view rendering (sf_hip_view.hip): one block for the key images, ray tables, large-sprite lists, argument tables and
    // output staging of a call, grown when a call needs more (dev_grow); the host copy
    // the tables are filled from; where the per-view list counters of the last call lie in the block
    unsigned char *view_scratch = nullptr;
    size_t view_bytes = 0;
    std::vector<unsigned char> view_tab_host;
    size_t view_counters_off = 0;
    int view_last_n = 0;
    // pose scoring (sf_hip_score.hip): a block of its own with the same drawing layout (ViewPlan) followed by the score
    // table, the result records and -- for the host-pointer calls -- the uploaded frames and the class images
    unsigned char *score_scratch = nullptr;
    size_t score_bytes = 0;
    std::vector<unsigned char> score_tab_host, score_args_host;  // the host copies of the view table and the score table
    // place recognition (sf_hip_keyframes.hip): live keyframe databases created from this handle: sf_destroy releases their
    // memory and orphans them, like the maps
    std::vector<struct sfk_db *> keyframe_dbs;
    // moving regions (sf_hip_regions.hip): one block for the entry table, the provisional label and count images, the block
    // counts and -- for the host forms -- the uploaded frames, records and label images of a call, grown when a call needs
    // more (dev_grow); the host copy the entry table is filled from
    unsigned char *regions_scratch = nullptr;
    size_t regions_bytes = 0;
    std::vector<unsigned char> regions_args_host;
    // pose refinement (sf_hip_align.hip): a block of its own with the drawing layout (ViewPlan) followed by the entry table
    // with the entries' states, the model images, the systems, the result records and -- for the host-pointer calls -- the
    // uploaded frames; the host copies of the view table and the entry table
    unsigned char *align_scratch = nullptr;
    size_t align_bytes = 0;
    std::vector<unsigned char> align_tab_host, align_args_host;
    // joined and thinned maps (sf_hip_join.hip): one block for the two entry tables, the counters, the voxel tables, the
    // remembered slots, the ballots and the block counts of a call, grown when a call needs more (dev_grow); the host copy
    // the tables are filled from
    unsigned char *join_scratch = nullptr;
    size_t join_bytes = 0;
    std::vector<unsigned char> join_args_host;
    // region tracks (sf_hip_tracks.hip): live trackers created from this handle. Their state and scratch are blocks of `own`;
    // sf_destroy releases them with it and orphans the trackers, like the keyframe databases
    std::vector<struct sft_tracker *> trackers;
    // region motion (sf_hip_bodies.hip): one block for the entry table, the pair table, the region states, the systems, the
    // model images and -- for the host form -- the uploaded frames and the results of a call, grown when a call needs more
    // (dev_grow); the host copies the two tables are filled from
    unsigned char *bodies_scratch = nullptr;
    size_t bodies_bytes = 0;
    std::vector<unsigned char> bodies_args_host;
    std::vector<int32_t> bodies_pairs_host;
    // body maps (sf_hip_body_maps.hip): one block for the two entry tables, the counters, the voxel tables with their bids, the
    // candidates' slots, the merge table, the ballots, the block counts and -- for the host form -- the uploaded frames of a
    // call, grown when a call needs more (dev_grow); the host copy the tables are filled from
    unsigned char *body_maps_scratch = nullptr;
    size_t body_maps_bytes = 0;
    std::vector<unsigned char> body_maps_args_host;
};

// the surfel map (sf_hip_model.hip creates, fuses and releases it; sf_hip_map_window.hip partitions it)
struct sf_map {
    sf_handle *h = nullptr;
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
    SfOwner own;    // the map's device blocks (not zero-filled): released by sf_map_destroy, or by its handle's sf_destroy
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
struct ViewPlan {
    int n = 0;
    std::vector<int> ray_of;     // per view: its ray table
    std::vector<int> ray_first;  // per ray table: the view that introduced it
    size_t off = 0;              // bytes laid out so far
    size_t o_tab = 0, o_rtab = 0, o_counters = 0, o_upload = 0;
    std::vector<size_t> o_rays, o_keys, o_list;
    size_t take(size_t bytes) {  // 256-byte aligned
        const size_t o = off;
        off = (off + bytes + 255) & ~(size_t)255;
        return o;
    }
};
SF_INTERNAL void sfv_plan(ViewPlan &p, int n, const ViewJob *jobs, const struct sfv_view *views, int upload_count);
SF_INTERNAL int sfv_draw_keys(sf_handle *h, const ViewPlan &p, const ViewJob *jobs, const struct sfv_view *views, const ViewOut *outs,
                              unsigned char *base, std::vector<unsigned char> &tab_host, const float *upload, int upload_count);
SF_INTERNAL void orphan_keyframe_dbs(sf_handle *h);  // sf_hip_keyframes.hip: sf_destroy releases the handle's keyframe databases
SF_INTERNAL void orphan_trackers(sf_handle *h);      // sf_hip_tracks.hip: sf_destroy leaves the handle's trackers as shells
// sf_hip_bodies.hip: the list of live handles (sf_create_ex enters a handle, sf_destroy takes it out), by which the region
// motion calls and the body map calls refuse a destroyed handle
SF_INTERNAL void handle_born(const sf_handle *h);
SF_INTERNAL void handle_gone(const sf_handle *h);
SF_INTERNAL bool handle_alive(const sf_handle *h);
extern "C" {  // (defined inside the extern "C" blocks of their files)
SF_INTERNAL int check_stream(const sf_handle *h, int stream);                 // sf_hip.hip
SF_INTERNAL int d2h(sf_handle *h, void *dst, const void *src, size_t bytes);  // sf_hip_solver.hip: drain the handle's stream, then copy
SF_INTERNAL int input_alloc(sf_handle *h);                                    // sf_hip_input.hip: buffers of the input stage, on first use
SF_INTERNAL void orphan_maps(sf_handle *h);                                   // sf_hip_model.hip: sf_destroy releases the handle's maps
SF_INTERNAL void invert_pose(const float pose[16], float out[16]);            // sf_hip_model.hip: t_inv of the prediction, the fusion and the views
// sf_hip_model.hip: a map handed to `what` beside h is not null (SF_ERR_ARG), not orphaned (SF_ERR_STATE) and h's own (SF_ERR_ARG)
SF_INTERNAL int check_map(const char *what, const sf_handle *h, const sf_map *m);
// sf_hip_model.hip: the table of a batched launch into h->tab_dev (grown on demand; it stays there for later launches of the call)
SF_INTERNAL int upload_table(sf_handle *h, const void *src, size_t bytes, void **dev);
SF_INTERNAL int results_scratch(sf_handle *h, size_t n_maps);                 // sf_hip_model.hip: h->res_dev holds 8 ints per batched map
}
