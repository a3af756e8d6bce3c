// sf_hip_migrate.hip — libsf_hip.so, the interface of include/sf_migrate.h (symbols sfm_*): single streams move between
// handles on the device, to and from host memory, or back to the state sf_create left. Kernels: sf_migrate.h; the layout of
// an exported stream and the ring rotation: sf_migrate_layout.h. No frame kernel is involved.
#include "../../include/sf_migrate.h"
#include "sf_host.h"
#include "sf_migrate.h"

#include <set>

extern "C" {

int sfm_version(void) { return SFM_VERSION; }

size_t sfm_blob_bytes(int rows, int cols, int levels, int with_input) {
    SfmLayout lay;
    return sfm_layout(rows, cols, levels, with_input, &lay) ? lay.total : 0;
}

}  // extern "C"

// Where segment `seg` of stream b lies in handle h, for a stream whose next frame is im_count (null: the handle has no such plane)
static void *segment_base(const sf_handle *h, int seg, int b, int im_count) {
    const KArgs &k = h->k;
    const size_t B = (size_t)k.batch, n0 = (size_t)k.n0, nt = (size_t)k.n_tot, sb = (size_t)b;
    if (seg == SFM_SEG_STATE) return k.state + sb;
    if (seg == SFM_SEG_STATS) return k.stats + sb;
    if (seg == SFM_SEG_PYR_NEW_D || seg == SFM_SEG_PYR_NEW_I) return k.pyr_new[seg - SFM_SEG_PYR_NEW_D] + sb * nt;
    if (seg == SFM_SEG_PYR_PRED_D || seg == SFM_SEG_PYR_PRED_I) return k.pyr_pred[seg - SFM_SEG_PYR_PRED_D] + sb * nt;
    if (seg == SFM_SEG_LABELS) return k.labels + sb * nt;
    if (seg == SFM_SEG_B_IMG) return k.b_img + sb * n0;
    if (seg >= SFM_SEG_HIST_D && seg < SFM_SEG_HIST_I) return k.hist_d + ((size_t)sfm_ring_slot(im_count, seg - SFM_SEG_HIST_D) * B + sb) * n0;
    if (seg >= SFM_SEG_HIST_I && seg < SFM_SEG_IN_DEPTH_MM) return k.hist_i + ((size_t)sfm_ring_slot(im_count, seg - SFM_SEG_HIST_I) * B + sb) * n0;
    if (!h->in_depth_mm) return nullptr;
    if (seg == SFM_SEG_IN_DEPTH_MM) return h->in_depth_mm + sb * n0;
    if (seg == SFM_SEG_IN_FILTERED_MM) return h->in_filtered_mm + sb * n0;
    if (seg == SFM_SEG_IN_DEPTH_METRIC) return h->in_depth_metric + sb * n0;
    if (seg == SFM_SEG_IN_COLOR) return h->in_color + sb * n0 * 3;
    return nullptr;
}

static int layout_of(const sf_handle *h, int with_input, SfmLayout *lay) {
    if (!sfm_layout(h->k.rows, h->k.cols, h->k.levels, with_input, lay) || lay->n0 != (size_t)h->k.n0 || lay->n_tot != (size_t)h->k.n_tot)
        return fail(SF_ERR_STATE, "sf_migrate_layout.h does not describe this handle's geometry");
    return SF_OK;
}

// The table of one call goes to the device through the next slot of the handle's ring (SfRing, sf_resources.h) on HIP stream
// `st`, without a host synchronisation: a slot is waited for only when the call four calls ago has not executed yet.
// The caller launches its kernel on `st` and then calls h->mig_ring.done(st).
static int table_upload(sf_handle *h, hipStream_t st, const void *entries, size_t bytes, void **dev) {
    const size_t cap = (size_t)h->k.batch * SFM_SEG_COUNT * SFM_ENTRY_BYTES;  // no call names more than every stream once
    if (bytes > cap) return fail(SF_ERR_ARG, "segment table larger than the handle");
    return h->mig_ring.next(h->own, cap, st, entries, bytes, dev);
}

static dim3 pair_grid(size_t pairs, size_t max_bytes) {
    // a block moves SFM_THREADS x SF_LOAD_BATCH 16-byte units per trip: about two trips per block, at most 16 blocks per segment
    const size_t per_trip = (size_t)SFM_THREADS * SF_LOAD_BATCH * 16;
    const unsigned gx = (unsigned)std::min<size_t>(16, std::max<size_t>(1, (max_bytes + 2 * per_trip - 1) / (2 * per_trip)));
    const unsigned gy = (unsigned)std::min<size_t>(pairs, 32768);
    return dim3(gx, gy, (unsigned)((pairs + gy - 1) / gy));
}

static int launch_copy(sf_handle *owner, hipStream_t st, const std::vector<SfmSeg> &segs) {
    void *dev = nullptr;
    if (int e = table_upload(owner, st, segs.data(), segs.size() * sizeof(SfmSeg), &dev)) return e;
    size_t max_bytes = 0;
    for (const SfmSeg &s : segs) max_bytes = std::max<size_t>(max_bytes, s.kind == SFM_KIND_BYTES ? s.bytes : 0);
    hipLaunchKernelGGL(sfm_copy_kernel, pair_grid(segs.size(), max_bytes), dim3(SFM_THREADS), 0, st, (const SfmSeg *)dev, (int)segs.size());
    HIP_TRY(hipGetLastError());
    return owner->mig_ring.done(st);
}

static int check_list(const sf_handle *h, const int *streams, int n, bool distinct, const char *what) {
    if (!streams) return fail(SF_ERR_ARG, std::string(what) + ": null stream list");
    std::set<int> seen;
    for (int q = 0; q < n; q++) {
        if (streams[q] < 0 || streams[q] >= h->k.batch) return fail(SF_ERR_ARG, std::string(what) + ": stream out of range");
        if (distinct && !seen.insert(streams[q]).second) return fail(SF_ERR_ARG, std::string(what) + ": a stream appears twice");
    }
    return SF_OK;
}

extern "C" {

int sfm_copy_streams(sf_handle *dst, const int *dst_streams, int dst_im_count, sf_handle *src, const int *src_streams, int src_im_count,
                     int n) {
    if (!dst || !src) return fail(SF_ERR_ARG, "sfm_copy_streams: null handle");
    if (n < 1) return fail(SF_ERR_ARG, "sfm_copy_streams: n < 1");
    if (dst->k.rows != src->k.rows || dst->k.cols != src->k.cols || dst->k.levels != src->k.levels)
        return fail(SF_ERR_ARG, "sfm_copy_streams: the handles differ in rows, cols or pyramid levels");
    if (dst->device != src->device) return fail(SF_ERR_ARG, "sfm_copy_streams: the handles are on different devices (export and import the stream instead)");
    if (!sfm_counts_compatible(src_im_count, dst_im_count))
        return fail(SF_ERR_ARG, "sfm_copy_streams: the frame counts must be equal, or both >= 5 (the residual stage needs five frames of history)");
    if (int e = check_list(dst, dst_streams, n, true, "sfm_copy_streams (destination)")) return e;
    if (int e = check_list(src, src_streams, n, false, "sfm_copy_streams (source)")) return e;
    if (src == dst) {
        const std::set<int> d(dst_streams, dst_streams + n);
        for (int q = 0; q < n; q++)
            if (d.count(src_streams[q])) return fail(SF_ERR_ARG, "sfm_copy_streams: within one handle a destination stream is also a source");
    }
    SfmLayout lay;
    const bool with_input = src->in_depth_mm != nullptr;
    if (int e = layout_of(src, with_input, &lay)) return e;
    HIP_TRY(hipSetDevice(dst->device));
    if (with_input)
        if (int e = input_alloc(dst)) return e;
    std::vector<SfmSeg> segs;
    segs.reserve((size_t)n * lay.segments);
    for (int q = 0; q < n; q++)
        for (int g = 0; g < lay.segments; g++) {
            SfmSeg s{};
            s.src = segment_base(src, g, src_streams[q], src_im_count);
            s.dst = segment_base(dst, g, dst_streams[q], dst_im_count);
            s.bytes = (unsigned)lay.bytes[g];
            s.kind = g == SFM_SEG_STATE ? SFM_KIND_STATE_TO_STATE : SFM_KIND_BYTES;
            s.src_count = src_im_count;
            s.dst_count = dst_im_count;
            segs.push_back(s);
        }
    // after everything queued on both handles, before everything queued later on either: an event each way, no host wait
    const bool two = src->stream != dst->stream;
    if (two) {
        for (sf_handle *q : {src, dst})
            if (!q->mig_ev)
                if (int e = q->own.event(&q->mig_ev, hipEventDisableTiming)) return e;
        HIP_TRY(hipEventRecord(src->mig_ev, src->stream));
        HIP_TRY(hipStreamWaitEvent(dst->stream, src->mig_ev, 0));
    }
    if (int e = launch_copy(dst, dst->stream, segs)) return e;
    if (two) {
        HIP_TRY(hipEventRecord(dst->mig_ev, dst->stream));
        HIP_TRY(hipStreamWaitEvent(src->stream, dst->mig_ev, 0));
    }
    if (with_input && src->have_frame) dst->have_frame = true;
    return SF_OK;
}

static int stage_for(sf_handle *h, size_t bytes) {
    return dev_grow(h, &h->mig_stage, &h->mig_stage_bytes, bytes);
}

int sfm_export_stream(sf_handle *h, int stream, int im_count, void *blob, size_t blob_bytes) {
    if (int e = check_stream(h, stream)) return e;
    if (!blob || im_count < 0) return fail(SF_ERR_ARG, "sfm_export_stream: bad argument");
    SfmLayout lay;
    const int with_input = h->in_depth_mm != nullptr;
    if (int e = layout_of(h, with_input, &lay)) return e;
    if (blob_bytes < lay.total) return fail(SF_ERR_ARG, "sfm_export_stream: blob_bytes is smaller than sfm_blob_bytes for this handle");
    HIP_TRY(hipSetDevice(h->device));
    if (int e = stage_for(h, lay.total)) return e;
    std::vector<SfmSeg> segs;
    for (int g = 0; g < lay.segments; g++) {
        SfmSeg s{};
        s.src = segment_base(h, g, stream, im_count);
        s.dst = h->mig_stage + lay.offset[g];
        s.bytes = (unsigned)lay.bytes[g];
        s.kind = g == SFM_SEG_STATE ? SFM_KIND_STATE_TO_PACK : SFM_KIND_BYTES;
        s.src_count = im_count;
        segs.push_back(s);
    }
    if (int e = launch_copy(h, h->stream, segs)) return e;
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy((char *)blob + SFM_HEADER_BYTES, h->mig_stage + SFM_HEADER_BYTES, lay.total - SFM_HEADER_BYTES, hipMemcpyDeviceToHost));
    SfmHeader hd{};
    hd.magic = SFM_MAGIC;
    hd.version = SFM_VERSION;
    hd.rows = h->k.rows;
    hd.cols = h->k.cols;
    hd.levels = h->k.levels;
    hd.with_input = with_input;
    hd.total_bytes = lay.total;
    static_assert(sizeof(SfmHeader) == SFM_HEADER_BYTES, "blob header");
    std::memcpy(blob, &hd, sizeof(hd));
    for (int g = 0; g < lay.segments; g++)  // the padding is zero whatever the staging block held
        std::memset((char *)blob + lay.offset[g] + lay.bytes[g], 0, sfm_pad16(lay.bytes[g]) - lay.bytes[g]);
    return SF_OK;
}

int sfm_import_stream(sf_handle *h, int stream, int im_count, const void *blob, size_t blob_bytes) {
    if (int e = check_stream(h, stream)) return e;
    if (!blob || im_count < 0) return fail(SF_ERR_ARG, "sfm_import_stream: bad argument");
    if (blob_bytes < SFM_HEADER_BYTES) return fail(SF_ERR_ARG, "sfm_import_stream: blob_bytes is smaller than a blob header");
    SfmHeader hd;
    std::memcpy(&hd, blob, sizeof(hd));
    if (hd.magic != SFM_MAGIC) return fail(SF_ERR_ARG, "sfm_import_stream: not an exported stream (magic)");
    if (hd.version != SFM_VERSION) return fail(SF_ERR_ARG, "sfm_import_stream: blob of another sfm_version");
    if (hd.rows != h->k.rows || hd.cols != h->k.cols || hd.levels != h->k.levels)
        return fail(SF_ERR_ARG, "sfm_import_stream: the blob's rows, cols or pyramid levels are not the handle's");
    if (hd.with_input != 0 && hd.with_input != 1) return fail(SF_ERR_ARG, "sfm_import_stream: bad header");
    SfmLayout lay;
    if (int e = layout_of(h, hd.with_input, &lay)) return e;
    if (hd.total_bytes != lay.total) return fail(SF_ERR_ARG, "sfm_import_stream: the blob's length field does not match its geometry");
    if (blob_bytes < lay.total) return fail(SF_ERR_ARG, "sfm_import_stream: blob_bytes is smaller than the blob");
    HIP_TRY(hipSetDevice(h->device));
    if (hd.with_input)
        if (int e = input_alloc(h)) return e;
    if (int e = stage_for(h, lay.total)) return e;
    HIP_TRY(hipMemcpyAsync(h->mig_stage + SFM_HEADER_BYTES, (const char *)blob + SFM_HEADER_BYTES, lay.total - SFM_HEADER_BYTES, hipMemcpyHostToDevice,
                           h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));  // the caller's buffer is free again
    std::vector<SfmSeg> segs;
    for (int g = 0; g < lay.segments; g++) {
        SfmSeg s{};
        s.src = h->mig_stage + lay.offset[g];
        s.dst = segment_base(h, g, stream, im_count);
        s.bytes = (unsigned)lay.bytes[g];
        s.kind = g == SFM_SEG_STATE ? SFM_KIND_PACK_TO_STATE : SFM_KIND_BYTES;
        s.dst_count = im_count;
        segs.push_back(s);
    }
    if (int e = launch_copy(h, h->stream, segs)) return e;
    if (hd.with_input) h->have_frame = true;
    return SF_OK;
}

int sfm_reset_streams(sf_handle *h, const int *streams, int n) {
    if (!h) return fail(SF_ERR_ARG, "sfm_reset_streams: null handle");
    if (n < 1) return fail(SF_ERR_ARG, "sfm_reset_streams: n < 1");
    if (int e = check_list(h, streams, n, true, "sfm_reset_streams")) return e;
    SfmLayout lay;
    if (int e = layout_of(h, h->in_depth_mm != nullptr, &lay)) return e;
    HIP_TRY(hipSetDevice(h->device));
    std::vector<SfmFill> fills;
    size_t max_bytes = 0;
    const float half = 0.5f;
    for (int q = 0; q < n; q++)
        for (int g = 0; g < lay.segments; g++) {
            SfmFill f{};
            f.dst = segment_base(h, g, streams[q], 0);
            f.bytes = (unsigned)lay.bytes[g];
            f.kind = g == SFM_SEG_STATE ? SFM_KIND_CTOR : SFM_KIND_FILL;
            if (g == SFM_SEG_B_IMG) std::memcpy(&f.pattern, &half, 4);  // b_segm_perpixel.fill(0.5f)
            f.kb = h->k.p.kb;
            fills.push_back(f);
            if (f.kind == SFM_KIND_FILL) max_bytes = std::max<size_t>(max_bytes, f.bytes);
        }
    void *dev = nullptr;
    if (int e = table_upload(h, h->stream, fills.data(), fills.size() * sizeof(SfmFill), &dev)) return e;
    hipLaunchKernelGGL(sfm_reset_kernel, pair_grid(fills.size(), max_bytes), dim3(SFM_THREADS), 0, h->stream, (const SfmFill *)dev, (int)fills.size());
    HIP_TRY(hipGetLastError());
    return h->mig_ring.done(h->stream);
}

}  // extern "C"
