/* sf_migrate.h — single streams between handles: move, checkpoint, reset.
 *
 * A companion of sf.h, not part of its ABI: plain C declarations with the prefix sfm_, exported by libsf_hip.so (and its
 * precise and reference-order builds) only. The CPU oracle does not implement them and SF_ABI_VERSION does not count them;
 * sfm_version() versions this interface and the blob format.
 *
 * A stream is bound to its slot of its handle from sf_create to sf_destroy. With these calls a service can
 *   - compact the live streams of a thinning batch into a smaller handle (sfm_copy_streams), so that sequences that have
 *     ended stop costing a solve per frame;
 *   - start new sequences in a small "nursery" handle and move them into a large one once their five-frame ring is full;
 *   - move one stream to a latency or cluster handle (the builds of source and destination may differ);
 *   - checkpoint streams to host memory and resume them on this or another device or process (sfm_export_stream /
 *     sfm_import_stream);
 *   - start a new sequence in a used slot (sfm_reset_streams).
 * No frame kernel takes part: a copy is one launch of a copy kernel for the whole set of streams.
 *
 * All functions return SF_OK or the SF_ERR_* codes of sf.h; sf_last_error() has the text.
 *
 * im_count: in every function, the number the caller will pass to the NEXT sf_process_frame on that handle. The library
 * does not track frame numbers, so the caller says it. A frame depends on im_count in two ways only: the ring slot it warps
 * from and overwrites is im_count % SF_HISTORY, and the residual stage runs when im_count >= SF_HISTORY. A stream may
 * therefore change phase when it moves: the ring entry of age a (0 = oldest .. 4) is slot (src_im_count + a) % 5 of the source
 * and lands in slot (dst_im_count + a) % 5 of the destination -- the depth and intensity rings and the pose ring alike. A
 * blob stores the entries in age order: its bytes do not depend on the stream index, the batch, the build or the phase.
 * A move is allowed when src_im_count == dst_im_count, or when both are >= SF_HISTORY (a young stream in a mature handle
 * would run the residual stage against history it never had): SF_ERR_ARG otherwise.
 *
 * WHAT TRAVELS: everything a later frame, a getter of sf.h, the prediction fill-in or a fuse reads from an earlier frame --
 * both pyramids (current and prediction; every level, depth and intensity), the labels of every level, the per-pixel b image,
 * the five entries of the depth / intensity ring, the stream's sf_frame_stats, the four images of the input stage
 * (sf_get_input_image) when the source handle has them (the destination allocates its own and counts as having a frame
 * loaded), and of the solver state: T_odometry, the three twists, the estimate covariance, b_segm, b_prior, lambda_t_w, the
 * K-means centres, the connectivity, the per-cluster residuals, the pose ring, kb (per stream: sf_set_kb), the level and
 * first-iteration mark and the pre-weight maxima of the last outer iteration.
 *
 * WHAT STAYS THE DESTINATION'S OWN (never overwritten): the rendezvous state of a cluster handle (a sticky
 * SF_STATUS_SYNC_TIMEOUT is the slot's, until sf_clear_sync_timeout), the record slot of the last iteration, and the totals
 * behind sf_get_counters / sf_get_stage_profile -- a handle counts what that handle solved. The solver parameters are the
 * destination handle's, except kb.
 *
 * WHAT DOES NOT TRAVEL:
 *   - the scratch of a single frame: warp accumulators, linearisation records, their label / Null planes, the source lists
 *     of the ordered splat and the debug planes. sf_get_lin_plane, sf_get_jacobian_rows and the SF_SET_WARPED / SF_SET_INTER
 *     planes of a migrated stream are therefore undefined until its next solve;
 *   - the per-stream density flag of the last prediction (sf_get_prediction_dense_stream): predict again;
 *   - data of a pending sf_upload_current_async: commit it before the move.
 *
 * REFUSALS (SF_ERR_ARG, nothing launched, nothing changed): rows, cols or pyramid levels differ; the handles are on
 * different devices (use a blob); an index out of range; an index twice among the destinations; src == dst and a
 * destination index also among the sources; n < 1; a blob with a wrong magic, version, geometry or length; blob_bytes too
 * small; sfm_map_rebind of a map whose handle was destroyed, or to a handle on another device or of another resolution.
 *
 * BLOB: a 64-byte header (uint32 magic "SFMB", uint32 sfm_version, int32 rows, cols, levels, with_input, uint64 total
 * bytes, 32 reserved zero bytes), then the segments in this order, each starting on a multiple of 16 bytes and padded with
 * zeros: solver state (347 32-bit words), sf_frame_stats, pyramid current depth, current intensity, prediction depth,
 * prediction intensity (n_tot floats each, n_tot = pixels of all levels), labels (n_tot bytes), b image (n0 floats,
 * n0 = rows * cols), depth ring (5 x n0 floats, oldest first), intensity ring (likewise), and with_input: depth mm, filtered
 * depth mm (n0 uint16 each), metric depth (n0 floats), colour (3 n0 bytes). Little endian, images column-major as in sf.h.
 */
#ifndef SF_MIGRATE_H_
#define SF_MIGRATE_H_

#include "sf.h"

#ifdef __cplusplus
extern "C" {
#endif

int sfm_version(void); /* 1 */

/* Pure host, no handle, no GPU: bytes of one exported stream of this geometry (levels = the handle's pyramid levels,
 * sf_get_params ctf_levels; with_input = the four input-stage images are included). 0 for a geometry no handle can have. */
size_t sfm_blob_bytes(int rows, int cols, int levels, int with_input);

/* Streams src_streams[0..n) of src -> streams dst_streams[0..n) of dst, entirely on the device, one launch for the whole
 * set. Asynchronous like sf_process_frame: it runs after everything already queued on BOTH handles' HIP streams, and work
 * queued on either handle after the call returns runs after the copy (events between the two HIP streams; the host does
 * not wait). A source stream may be named several times; src == dst is allowed when no destination is also a source. Both
 * handles stay alive and usable: during a compaction both occupy memory. */
int sfm_copy_streams(sf_handle *dst, const int *dst_streams, int dst_im_count,
                     sf_handle *src, const int *src_streams, int src_im_count, int n);

/* One stream <-> host memory. Both return when `blob` may be reused; the import's write into the handle is queued on
 * its HIP stream like any other call. An export with input images happens when the handle has used the input stage. */
int sfm_export_stream(sf_handle *h, int stream, int im_count, void *blob, size_t blob_bytes);
int sfm_import_stream(sf_handle *h, int stream, int im_count, const void *blob, size_t blob_bytes);

/* The named streams back to what sf_create left: slots ready for a new sequence at im_count 0 (kb: the handle's
 * parameter). Asynchronous on the handle's HIP stream. */
int sfm_reset_streams(sf_handle *h, const int *streams, int n);

/* A surfel map follows its stream: the map now belongs to dst (same device, same rows x cols) -- dst is the handle to name
 * in sf_map_fuse_frame / sf_map_predict from now on, and destroying the old handle no longer releases the map. Waits for
 * the old handle's queued work. The map's memory is its own and does not move. */
int sfm_map_rebind(sf_map *m, sf_handle *dst);

#ifdef __cplusplus
}
#endif
#endif
