/* sf_keyframes.h — place recognition: fern-coded keyframes that propose poses.
 *
 * A companion of sf.h, not part of its ABI: plain C declarations with the prefix sfk_, exported by libsf_hip.so (and its
 * precise and reference-order builds) only. The CPU oracle does not implement them and SF_ABI_VERSION does not count them;
 * sfk_version() versions this interface.
 *
 * sf_score.h tells a caller that a stream is lost and ranks candidate poses once it has some. These calls produce the
 * candidates: "which earlier view does the current frame look like?", on the device, for many streams per call. A frame is
 * reduced to a short code by randomised ferns (Glocker et al.; ElasticFusion's Ferns); a database keeps the codes of the
 * keyframes with the poses they were seen from; a query returns the stored slots whose codes differ least. The poses of the
 * matches go to sfs_score_streams, and the solver's own frame-to-model step refines from the winner.
 * Everything below is stated on integers, so a code, a distance and a result are functions of their inputs alone: the same
 * for any batch composition, any summation order and from run to run.
 *
 * GRID AND CELLS. A database is made for one image size rows x cols (1..4096 each) and one cell size `cell` (1..64). The
 * grid is gr = rows / cell by gc = cols / cell (integer division); pixels beyond gr * cell rows or gc * cell columns are
 * never read. gr * gc must lie in 1..4096. Cell (cv, cu) has the index c = cv + cu * gr.
 *
 * IMAGES are column-major float32 like every image of sf.h: element (v, u) at v + u * rows. zf is depth, gf is grey.
 *
 * THUMBNAIL. Per cell, over its a = cell * cell pixels; a comparison with a NaN operand is false:
 *   n = the number of pixels with zf > 0
 *   Z = the sum over those pixels of (int32)rintf(fminf(zf, 32.f) * 1024.f)
 *   G = the sum over all a pixels of (int32)rintf(fminf(fmaxf(gf, 0.f), 1.f) * 4096.f)
 * fmaxf and fminf return their other operand when one is a NaN, so a NaN grey adds 0 and +inf adds 4096; +inf depth counts
 * as valid and adds 32768. Everything fits int32: Z <= 2^27, G <= 2^24.
 *
 * FERN. 0 <= cell < gr * gc, 0 <= t_grey <= 4096, 0 <= t_depth <= 32768. Its 4-bit code on a frame:
 *   bit0 = G > t_grey * a
 *   bit1 = n > 0 && Z > t_depth * n
 *   bit2 = 2 * n >= a
 *   bit3 = 0
 *
 * CODE of a frame: words = (n_ferns + 7) / 8 uint32, n_ferns in 1..4096. Fern f sits in bits 4 * (f % 8) .. 4 * (f % 8) + 3
 * of word f / 8; unused nibbles are 0.
 *
 * DISTANCE of two codes: the number of ferns whose nibbles differ, 0..n_ferns.
 *
 * A DATABASE (sfk_db) belongs to the handle it was created from and is ordered on that handle's HIP stream. It holds up to
 * `capacity` slots (1..1048576), filled from slot 0: a code, a pose (16 floats, copied and never interpreted), a tag
 * (int32 >= 0: the caller's name for the map or place the keyframe belongs to) and a stamp (int32, the caller's). Codes and
 * tags lie in device memory, codes word by word so that neighbouring slots are neighbouring addresses; poses and stamps,
 * which no kernel reads, lie in host memory. sfk_db_destroy destroys a database; its handle's sf_destroy releases its
 * memory and leaves an empty shell on which every call but sfk_db_destroy returns SF_ERR_STATE.
 *
 * All functions return SF_OK or the SF_ERR_* codes of sf.h; sf_last_error() has the text.
 *
 * REFUSALS (SF_ERR_ARG unless said otherwise; nothing launched, nothing written): a null argument; n < 0 (n == 0 is SF_OK);
 * n > 65535; every range named above; a database of a destroyed handle (SF_ERR_STATE); a database whose rows and cols are not
 * the handle's, in the stream forms; a stream index out of range (the code of sf_get_current); a fern out of range; m
 * outside 1..16; a negative min_distance; first + n > count in sfk_db_get; count > capacity in sfk_db_set; a negative tag in
 * add or set; two equal tags in one add call; count + novel > capacity in add (SF_ERR_STATE, nothing changes); scratch that
 * cannot be allocated (SF_ERR_NOMEM).
 *
 * NOT HERE: a per-tag index for the search (every query reads every slot), removal of single slots, colour ferns (the
 * streams keep grey only).
 */
#ifndef SF_KEYFRAMES_H_
#define SF_KEYFRAMES_H_

#include "sf.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sfk_db sfk_db;

typedef struct sfk_fern {
    int32_t cell;      /* 0 <= . < grid_rows * grid_cols */
    int32_t t_grey;    /* 0 .. 4096: mean grey of the cell in 1/4096 */
    int32_t t_depth;   /* 0 .. 32768: mean depth of the cell's valid pixels in 1/1024 m */
    int32_t reserved;  /* not read */
} sfk_fern;            /* 16 bytes; sfk_fern_bytes() reports it */

typedef struct sfk_match {
    int32_t slot;      /* -1: no such slot */
    int32_t distance;  /* -1 with slot -1 */
} sfk_match;           /* 8 bytes; sfk_match_bytes() reports it */

typedef struct sfk_info {
    int32_t rows, cols, cell, grid_rows, grid_cols, n_ferns, words, capacity, count;
    int32_t reserved[3];  /* written as 0 */
} sfk_info;               /* 48 bytes; sfk_info_bytes() reports it */

int sfk_version(void); /* 1 */
size_t sfk_fern_bytes(void);  /* sizeof(sfk_fern) = 16 */
size_t sfk_match_bytes(void); /* sizeof(sfk_match) = 8 */
size_t sfk_info_bytes(void);  /* sizeof(sfk_info) = 48 */

/* Pure host, integer only. x = seed (uint64); next() does x = 6364136223846793005 * x + 1442695040888963407 mod 2^64 and
 * returns x >> 33. For each fern in order: cell = next() % n_cells, t_grey = 410 + next() % 3277, t_depth = 512 + next() % 6656
 * (grey 0.1 .. 0.9, depth 0.5 .. 7 m); reserved = 0. SF_ERR_ARG: null, n_ferns outside 1..4096, n_cells outside 1..4096. */
int sfk_default_ferns(int n_ferns, uint64_t seed, int n_cells, sfk_fern *out);

/* Pure host: SF_OK, or SF_ERR_ARG for null, n_ferns outside 1..4096, n_cells outside 1..4096 or a fern out of range. */
int sfk_check_ferns(const sfk_fern *ferns, int n_ferns, int n_cells);

int sfk_db_create(sf_handle *h, int rows, int cols, int cell, const sfk_fern *ferns, int n_ferns, int capacity, sfk_db **out);
void sfk_db_destroy(sfk_db *db);
int sfk_db_info(const sfk_db *db, sfk_info *info);
int sfk_db_clear(sfk_db *db); /* count = 0 */

/* Slots first .. first + n - 1 to HOST memory: codes [n][words] uint32, poses [n][16], tags [n], stamps [n]; any output may
 * be NULL. Returns after the handle's stream has drained. */
int sfk_db_get(sfk_db *db, int first, int n, uint32_t *codes, float *poses, int32_t *tags, int32_t *stamps);

/* Replaces the content by `count` slots from HOST memory, laid out as sfk_db_get returns them: with it the checkpoint /
 * resume pair. get -> set into a fresh database of the same size and ferns reproduces every later result. */
int sfk_db_set(sfk_db *db, int count, const uint32_t *codes, const float *poses, const int32_t *tags, const int32_t *stamps);

/* ENCODE, n <= 65535 entries in one set of launches. codes_out is HOST memory, [n][words].
 * _streams: entry q is the current frame of streams[q] of the database's handle -- the level-0 depth and intensity
 * sf_get_current returns, read on the device where they lie, exactly what sfs_score_streams reads.
 * _images: depth[q] and grey[q] are HOST images of the database's size.
 * _images_device: DEVICE pointers in the (host) arrays depth and grey, d_codes ONE device pointer to [n][words]; asynchronous
 * on the handle's stream, nothing is read back. */
int sfk_encode_streams(sfk_db *db, int n, const int32_t *streams, uint32_t *codes_out);
int sfk_encode_images(sfk_db *db, int n, const float *const *depth, const float *const *grey, uint32_t *codes_out);
int sfk_encode_images_device(sfk_db *db, int n, const void *const *depth, const void *const *grey, void *d_codes);

/* QUERY. For entry q the m best slots (1 <= m <= 16) among the slots considered: every slot when tags[q] < 0, else the
 * slots whose tag equals tags[q]. The result is the m smallest (distance, slot) pairs in ascending lexicographic order --
 * an equal distance goes to the lower slot --, places that have no slot are {-1, -1}. matches_out is HOST memory,
 * [n][m]. The same stream or code may appear any number of times. A query only READS: afterwards the database, the streams,
 * the maps, the view scratch and the score scratch are what they were. */
int sfk_query_streams(sfk_db *db, int n, const int32_t *streams, const int32_t *tags, int m, sfk_match *matches_out);
int sfk_query_codes(sfk_db *db, int n, const uint32_t *codes, const int32_t *tags, int m, sfk_match *matches_out);

/* ADD. Entry q is NOVEL when no slot with its tag exists, or the smallest distance to the slots with its tag is
 * >= min_distance (0: always add). Novel entries are appended in the order of q; slots_out[q] is the new slot, or -1.
 * nearest_out is NULL or receives the best same-tag match BEFORE the call, or {-1, -1}. poses is [n][16]. The tags of one
 * call are >= 0 and pairwise distinct, so its entries do not depend on one another. count + novel > capacity is
 * SF_ERR_STATE and nothing changes. Synchronous: distances on the device, flags read back, slots assigned on the host, then
 * the codes (already on the device), poses, tags and stamps stored. */
int sfk_add_streams(sfk_db *db, int n, const int32_t *streams, const float *poses, const int32_t *tags, const int32_t *stamps,
                    int min_distance, int32_t *slots_out, sfk_match *nearest_out);
int sfk_add_codes(sfk_db *db, int n, const uint32_t *codes, const float *poses, const int32_t *tags, const int32_t *stamps,
                  int min_distance, int32_t *slots_out, sfk_match *nearest_out);

#ifdef __cplusplus
}
#endif
#endif
