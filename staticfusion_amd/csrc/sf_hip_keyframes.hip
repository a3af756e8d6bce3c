// sf_hip_keyframes.hip — libsf_hip.so, the interface of include/sf_keyframes.h (symbols sfk_*): fern codes of frames, a
// database of coded keyframes with their poses, the search of it and the adding to it (kernels: sf_keyframes.h). A database
// owns its device blocks (ferns, codes, tags, and the call block sfk_db::scratch: sf_call_block.h) through an owner of its
// own, as a map does; its handle's sf_destroy releases them and leaves an empty shell. Poses and stamps, which no kernel reads, are
// host vectors. Every call checks everything before it launches or writes anything.
#include "../../include/sf_keyframes.h"
#include "sf_host.h"
#include "sf_keyframes.h"

#define SFK_VERSION 1
static_assert(sizeof(sfk_fern) == 16, "include/sf_keyframes.h: sfk_fern is 16 bytes");
static_assert(sizeof(sfk_match) == 8, "include/sf_keyframes.h: sfk_match is 8 bytes");
static_assert(sizeof(sfk_info) == 48, "include/sf_keyframes.h: sfk_info is 48 bytes");

struct SF_INTERNAL sfk_db : SfPart {
    int rows = 0, cols = 0, cell = 0, gr = 0, gc = 0, n_ferns = 0, words = 0, capacity = 0, count = 0;
    sfk_fern *d_ferns = nullptr;
    uint32_t *d_codes = nullptr;  // [words][capacity]: word w of slot s at w * capacity + s
    int32_t *d_tags = nullptr;    // [capacity]
    std::vector<float> poses;     // [count][16]
    std::vector<int32_t> stamps;  // [count]
    SfCallBlock scratch;          // what one call uploads, encodes and reads back; host copy 0: the frame table
    void shelled() override {
        scratch.forget();
        d_ferns = nullptr;
        d_codes = nullptr;
        d_tags = nullptr;
    }
};

static int check_ferns(const sfk_fern *ferns, int n_ferns, int n_cells) {
    if (!ferns) return fail(SF_ERR_ARG, "sfk: null ferns");
    if (n_ferns < 1 || n_ferns > 4096) return fail(SF_ERR_ARG, "sfk: n_ferns lies in 1..4096");
    if (n_cells < 1 || n_cells > 4096) return fail(SF_ERR_ARG, "sfk: the number of cells lies in 1..4096");
    for (int f = 0; f < n_ferns; f++)
        if (ferns[f].cell < 0 || ferns[f].cell >= n_cells || ferns[f].t_grey < 0 || ferns[f].t_grey > 4096 || ferns[f].t_depth < 0 || ferns[f].t_depth > 32768)
            return fail(SF_ERR_ARG, "sfk: fern " + std::to_string(f) + " out of range");
    return SF_OK;
}

static int check_db(const char *what, const sfk_db *db) { return check_part(what, db, "database"); }

static int check_streams(const char *what, const sfk_db *db, int n, const int32_t *streams) {
    const sf_handle *h = db->h;
    if (db->rows != h->k.rows || db->cols != h->k.cols) return fail(SF_ERR_ARG, std::string(what) + ": a database of another size than the handle's streams");
    for (int q = 0; q < n; q++)
        if (int e = check_stream(h, streams[q])) return e;  // where sf_get_current refuses, with its code
    return SF_OK;
}

// ---- a call's scratch block (under the database's own owner) and the launches ------------------------------------------
static int grow_scratch(sfk_db *db, size_t bytes) { return db->scratch.grow(db->own, bytes, db->h->stream); }

// frames -> codes [n][words] at d_codes, on the handle's stream. The frame table lies at o_frames of the scratch block; the
// host images of FORM_HOST are uploaded to o_images (n x 2 images). Everything has been checked and the block has been grown.
static int encode(sfk_db *db, CallForm form, int n, const int32_t *streams, const void *const *depth, const void *const *grey, size_t o_frames,
                  size_t o_images, uint32_t *d_codes) {
    sf_handle *h = db->h;
    const size_t px = (size_t)db->rows * db->cols;
    KfFrame *frames = db->scratch.resized<KfFrame>((size_t)n);
    uintptr_t bits = 0;  // the alignment of every image of the call
    for (int q = 0; q < n; q++) {
        KfFrame &f = frames[(size_t)q];
        if (form == FORM_STREAMS) {
            f.depth = h->k.pyr_new[0] + (size_t)streams[q] * h->k.n_tot;  // what sf_get_current copies out and sfs_score_streams reads
            f.grey = h->k.pyr_new[1] + (size_t)streams[q] * h->k.n_tot;
        } else if (form == FORM_HOST) {
            float *d = (float *)(db->scratch.dev + o_images) + (size_t)q * 2 * px;
            HIP_TRY(hipMemcpyAsync(d, depth[q], px * 4, hipMemcpyHostToDevice, h->stream));
            HIP_TRY(hipMemcpyAsync(d + px, grey[q], px * 4, hipMemcpyHostToDevice, h->stream));
            f.depth = d;
            f.grey = d + px;
        } else {
            f.depth = (const float *)depth[q];
            f.grey = (const float *)grey[q];
        }
        bits |= (uintptr_t)f.depth | (uintptr_t)f.grey;
    }
    KfFrame *d_frames = (KfFrame *)(db->scratch.dev + o_frames);
    if (int e = db->scratch.upload(o_frames, frames, (size_t)n * sizeof(KfFrame), h->stream)) return e;
    // the widest load: W floats that never straddle a cell, start on a multiple of W in every column, and are aligned
    int w = 1;
    if (db->cell % 4 == 0 && db->rows % 4 == 0 && bits % 16 == 0) w = 4;
    else if (db->cell % 2 == 0 && db->rows % 2 == 0 && bits % 8 == 0) w = 2;
    const KfGeom g = kf_geometry(db->rows, db->cell, db->gr, db->gc, w);
    const size_t lds = (size_t)3 * db->gr * db->gc * sizeof(int);
    auto kernel = w == 4 ? sfk_encode_kernel<4> : w == 2 ? sfk_encode_kernel<2> : sfk_encode_kernel<1>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)n), dim3(SFK_NT), lds, h->stream, (const KfFrame *)d_frames, (const sfk_fern *)db->d_ferns, db->n_ferns,
                       db->words, g, d_codes);
    HIP_TRY(hipGetLastError());
    return SF_OK;
}

// the m best slots of n codes at d_codes under the tags at d_tags -> d_out [n][m]
static int search(sfk_db *db, int n, const uint32_t *d_codes, const int32_t *d_tags, int m, sfk_match *d_out) {
    const size_t lds = ((size_t)m * SFK_NT + SFK_NT / 64) * sizeof(unsigned long long) + (size_t)db->words * sizeof(uint32_t);
    hipLaunchKernelGGL(sfk_query_kernel, dim3((unsigned)n), dim3(SFK_NT), lds, db->h->stream, (const uint32_t *)db->d_codes, (const int32_t *)db->d_tags,
                       db->capacity, db->count, db->words, d_codes, d_tags, m, d_out);
    HIP_TRY(hipGetLastError());
    return SF_OK;
}

static int encode_to_host(const char *what, CallForm form, sfk_db *db, int n, const int32_t *streams, const float *const *depth, const float *const *grey,
                          uint32_t *codes_out) {
    if (int e = check_db(what, db)) return e;
    if (int e = check_batch(what, n)) return e;
    if (n == 0) return SF_OK;
    if (!codes_out || (form == FORM_STREAMS ? !streams : (!depth || !grey))) return fail(SF_ERR_ARG, std::string(what) + ": null argument");
    if (form == FORM_STREAMS) {
        if (int e = check_streams(what, db, n, streams)) return e;
    } else {
        for (int q = 0; q < n; q++)
            if (!depth[q] || !grey[q]) return fail(SF_ERR_ARG, std::string(what) + ": null image");
    }
    sf_handle *h = db->h;
    HIP_TRY(hipSetDevice(h->device));
    SfPlan p;
    const size_t o_frames = p.take((size_t)n * sizeof(KfFrame));
    const size_t o_codes = p.take((size_t)n * db->words * 4);
    const size_t o_images = form == FORM_HOST ? p.take((size_t)n * 2 * db->rows * db->cols * 4) : 0;
    if (int e = grow_scratch(db, p.off)) return e;
    uint32_t *d_codes = (uint32_t *)(db->scratch.dev + o_codes);
    if (int e = encode(db, form, n, streams, (const void *const *)depth, (const void *const *)grey, o_frames, o_images, d_codes)) return e;
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(codes_out, d_codes, (size_t)n * db->words * 4, hipMemcpyDeviceToHost));
    return SF_OK;
}

static int check_tags(const char *what, int n, const int32_t *tags) {  // of an add call: >= 0 and pairwise distinct
    std::vector<int32_t> t(tags, tags + n);
    std::sort(t.begin(), t.end());
    if (t[0] < 0) return fail(SF_ERR_ARG, std::string(what) + ": a negative tag");
    for (int q = 1; q < n; q++)
        if (t[(size_t)q] == t[(size_t)q - 1]) return fail(SF_ERR_ARG, std::string(what) + ": the same tag twice in one call");
    return SF_OK;
}

// streams (codes == null) or host codes: query (slots == null) or add
static int query_or_add(const char *what, sfk_db *db, int n, const int32_t *streams, const uint32_t *codes, bool from_streams, const int32_t *tags, int m,
                        sfk_match *matches_out, bool add, const float *poses, const int32_t *stamps, int min_distance, int32_t *slots_out) {
    if (int e = check_db(what, db)) return e;
    if (int e = check_batch(what, n)) return e;
    if (n == 0) return SF_OK;
    if (!tags || (from_streams ? !streams : !codes)) return fail(SF_ERR_ARG, std::string(what) + ": null argument");
    if (add) {
        if (!poses || !stamps || !slots_out) return fail(SF_ERR_ARG, std::string(what) + ": null argument");
        if (min_distance < 0) return fail(SF_ERR_ARG, std::string(what) + ": a negative min_distance");
        if (int e = check_tags(what, n, tags)) return e;
    } else {
        if (!matches_out) return fail(SF_ERR_ARG, std::string(what) + ": null argument");
        if (m < 1 || m > 16) return fail(SF_ERR_ARG, std::string(what) + ": m lies in 1..16");
    }
    if (from_streams)
        if (int e = check_streams(what, db, n, streams)) return e;
    sf_handle *h = db->h;
    HIP_TRY(hipSetDevice(h->device));
    const size_t code_bytes = (size_t)n * db->words * 4;
    SfPlan p;
    const size_t o_frames = p.take((size_t)n * sizeof(KfFrame));
    const size_t o_codes = p.take(code_bytes);
    const size_t o_tags = p.take((size_t)n * 4);
    const size_t o_match = p.take((size_t)n * m * sizeof(sfk_match));
    const size_t o_slots = p.take((size_t)n * 4);
    if (int e = grow_scratch(db, p.off)) return e;
    uint32_t *d_codes = (uint32_t *)(db->scratch.dev + o_codes);
    int32_t *d_tags = (int32_t *)(db->scratch.dev + o_tags), *d_slots = (int32_t *)(db->scratch.dev + o_slots);
    sfk_match *d_match = (sfk_match *)(db->scratch.dev + o_match);
    if (from_streams) {
        if (int e = encode(db, FORM_STREAMS, n, streams, nullptr, nullptr, o_frames, 0, d_codes)) return e;
    } else {
        HIP_TRY(hipMemcpyAsync(d_codes, codes, code_bytes, hipMemcpyHostToDevice, h->stream));
    }
    HIP_TRY(hipMemcpyAsync(d_tags, tags, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    if (int e = search(db, n, d_codes, d_tags, m, d_match)) return e;
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (!add) {
        HIP_TRY(hipMemcpy(matches_out, d_match, (size_t)n * m * sizeof(sfk_match), hipMemcpyDeviceToHost));
        return SF_OK;
    }
    // ---- add: flags back, slots on the host, then the store
    std::vector<sfk_match> nearest((size_t)n);
    HIP_TRY(hipMemcpy(nearest.data(), d_match, (size_t)n * sizeof(sfk_match), hipMemcpyDeviceToHost));
    std::vector<int32_t> slots((size_t)n);
    int next = db->count;
    for (int q = 0; q < n; q++) {
        const bool novel = nearest[(size_t)q].slot < 0 || nearest[(size_t)q].distance >= min_distance;
        slots[(size_t)q] = novel ? next++ : -1;
    }
    if (next > db->capacity) return fail(SF_ERR_STATE, std::string(what) + ": the database is full (count + novel entries > capacity)");
    if (next > db->count) {
        HIP_TRY(hipMemcpyAsync(d_slots, slots.data(), (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
        const long long items = (long long)n * db->words;
        hipLaunchKernelGGL(sfk_store_kernel, dim3((unsigned)((items + SFK_NT - 1) / SFK_NT)), dim3(SFK_NT), 0, h->stream, (const uint32_t *)d_codes,
                           (const int32_t *)d_slots, (const int32_t *)d_tags, n, db->words, db->d_codes, db->d_tags, db->capacity);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(h->stream));  // (slots is a local)
        db->poses.resize((size_t)next * 16);
        db->stamps.resize((size_t)next);
        for (int q = 0; q < n; q++)
            if (slots[(size_t)q] >= 0) {
                std::memcpy(&db->poses[(size_t)slots[(size_t)q] * 16], poses + (size_t)q * 16, 16 * sizeof(float));
                db->stamps[(size_t)slots[(size_t)q]] = stamps[q];
            }
        db->count = next;
    }
    std::memcpy(slots_out, slots.data(), (size_t)n * 4);
    if (matches_out) std::memcpy(matches_out, nearest.data(), (size_t)n * sizeof(sfk_match));
    return SF_OK;
}

extern "C" {

int sfk_version(void) { return SFK_VERSION; }
size_t sfk_fern_bytes(void) { return sizeof(sfk_fern); }
size_t sfk_match_bytes(void) { return sizeof(sfk_match); }
size_t sfk_info_bytes(void) { return sizeof(sfk_info); }

int sfk_default_ferns(int n_ferns, uint64_t seed, int n_cells, sfk_fern *out) {
    if (!out) return fail(SF_ERR_ARG, "sfk_default_ferns: null");
    if (n_ferns < 1 || n_ferns > 4096) return fail(SF_ERR_ARG, "sfk_default_ferns: n_ferns lies in 1..4096");
    if (n_cells < 1 || n_cells > 4096) return fail(SF_ERR_ARG, "sfk_default_ferns: the number of cells lies in 1..4096");
    uint64_t x = seed;
    auto next = [&x]() {
        x = 6364136223846793005ull * x + 1442695040888963407ull;
        return x >> 33;
    };
    for (int f = 0; f < n_ferns; f++) {
        out[f].cell = (int32_t)(next() % (uint64_t)n_cells);
        out[f].t_grey = 410 + (int32_t)(next() % 3277);
        out[f].t_depth = 512 + (int32_t)(next() % 6656);
        out[f].reserved = 0;
    }
    return SF_OK;
}

int sfk_check_ferns(const sfk_fern *ferns, int n_ferns, int n_cells) { return check_ferns(ferns, n_ferns, n_cells); }

int sfk_db_create(sf_handle *h, int rows, int cols, int cell, const sfk_fern *ferns, int n_ferns, int capacity, sfk_db **out) {
    if (!h || !out) return fail(SF_ERR_ARG, "sfk_db_create: null argument");
    if (rows < 1 || rows > 4096 || cols < 1 || cols > 4096) return fail(SF_ERR_ARG, "sfk_db_create: rows and cols lie in 1..4096");
    if (cell < 1 || cell > 64) return fail(SF_ERR_ARG, "sfk_db_create: cell lies in 1..64");
    const int gr = rows / cell, gc = cols / cell;
    if (gr * gc < 1 || gr * gc > 4096) return fail(SF_ERR_ARG, "sfk_db_create: the grid has 1..4096 cells");
    if (int e = check_ferns(ferns, n_ferns, gr * gc)) return e;
    if (capacity < 1 || capacity > 1048576) return fail(SF_ERR_ARG, "sfk_db_create: capacity lies in 1..1048576");
    HIP_TRY(hipSetDevice(h->device));
    sfk_db *db = new sfk_db;
    db->rows = rows; db->cols = cols; db->cell = cell; db->gr = gr; db->gc = gc;
    db->n_ferns = n_ferns; db->words = (n_ferns + 7) / 8; db->capacity = capacity;
    int e = db->own.device(&db->d_ferns, (size_t)n_ferns);
    if (!e) e = db->own.device(&db->d_codes, (size_t)db->words * capacity);
    if (!e) e = db->own.device(&db->d_tags, (size_t)capacity);
    if (!e && hipMemcpy(db->d_ferns, ferns, (size_t)n_ferns * sizeof(sfk_fern), hipMemcpyHostToDevice) != hipSuccess) e = fail(SF_ERR_DEVICE, "sfk_db_create: hipMemcpy");
    if (e) {
        delete db;  // (its owner releases what it had)
        return e;
    }
    db->h = h;
    h->parts.enter(db);
    *out = db;
    return SF_OK;
}

void sfk_db_destroy(sfk_db *db) {
    if (!db) return;
    part_destroy(db);
    delete db;
}

int sfk_db_info(const sfk_db *db, sfk_info *info) {
    if (int e = check_db("sfk_db_info", db)) return e;
    if (!info) return fail(SF_ERR_ARG, "sfk_db_info: null");
    *info = sfk_info{db->rows, db->cols, db->cell, db->gr, db->gc, db->n_ferns, db->words, db->capacity, db->count, {0, 0, 0}};
    return SF_OK;
}

int sfk_db_clear(sfk_db *db) {
    if (int e = check_db("sfk_db_clear", db)) return e;
    db->count = 0;
    db->poses.clear();
    db->stamps.clear();
    return SF_OK;
}

int sfk_db_get(sfk_db *db, int first, int n, uint32_t *codes, float *poses, int32_t *tags, int32_t *stamps) {
    if (int e = check_db("sfk_db_get", db)) return e;
    if (first < 0 || n < 0 || (long long)first + n > db->count) return fail(SF_ERR_ARG, "sfk_db_get: first + n > count");
    if (n == 0) return SF_OK;
    sf_handle *h = db->h;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (codes) {  // [words][capacity] on the device -> [slot][words]
        std::vector<uint32_t> by_word((size_t)db->words * n);
        HIP_TRY(hipMemcpy2D(by_word.data(), (size_t)n * 4, db->d_codes + first, (size_t)db->capacity * 4, (size_t)n * 4, (size_t)db->words, hipMemcpyDeviceToHost));
        for (int s = 0; s < n; s++)
            for (int w = 0; w < db->words; w++) codes[(size_t)s * db->words + w] = by_word[(size_t)w * n + s];
    }
    if (tags) HIP_TRY(hipMemcpy(tags, db->d_tags + first, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (poses) std::memcpy(poses, &db->poses[(size_t)first * 16], (size_t)n * 16 * sizeof(float));
    if (stamps) std::memcpy(stamps, &db->stamps[(size_t)first], (size_t)n * 4);
    return SF_OK;
}

int sfk_db_set(sfk_db *db, int count, const uint32_t *codes, const float *poses, const int32_t *tags, const int32_t *stamps) {
    if (int e = check_db("sfk_db_set", db)) return e;
    if (count < 0 || count > db->capacity) return fail(SF_ERR_ARG, "sfk_db_set: count > capacity");
    if (count > 0 && (!codes || !poses || !tags || !stamps)) return fail(SF_ERR_ARG, "sfk_db_set: null argument");
    for (int s = 0; s < count; s++)
        if (tags[s] < 0) return fail(SF_ERR_ARG, "sfk_db_set: a negative tag");
    sf_handle *h = db->h;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (count > 0) {
        std::vector<uint32_t> by_word((size_t)db->words * count);
        for (int s = 0; s < count; s++)
            for (int w = 0; w < db->words; w++) by_word[(size_t)w * count + s] = codes[(size_t)s * db->words + w];
        HIP_TRY(hipMemcpy2D(db->d_codes, (size_t)db->capacity * 4, by_word.data(), (size_t)count * 4, (size_t)count * 4, (size_t)db->words, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(db->d_tags, tags, (size_t)count * 4, hipMemcpyHostToDevice));
    }
    db->poses.assign(poses, poses + (size_t)count * 16);
    db->stamps.assign(stamps, stamps + (size_t)count);
    db->count = count;
    return SF_OK;
}

int sfk_encode_streams(sfk_db *db, int n, const int32_t *streams, uint32_t *codes_out) {
    return encode_to_host("sfk_encode_streams", FORM_STREAMS, db, n, streams, nullptr, nullptr, codes_out);
}

int sfk_encode_images(sfk_db *db, int n, const float *const *depth, const float *const *grey, uint32_t *codes_out) {
    return encode_to_host("sfk_encode_images", FORM_HOST, db, n, nullptr, depth, grey, codes_out);
}

int sfk_encode_images_device(sfk_db *db, int n, const void *const *depth, const void *const *grey, void *d_codes) {
    const char *what = "sfk_encode_images_device";
    if (int e = check_db(what, db)) return e;
    if (int e = check_batch(what, n)) return e;
    if (n == 0) return SF_OK;
    if (!depth || !grey || !d_codes) return fail(SF_ERR_ARG, std::string(what) + ": null argument");
    for (int q = 0; q < n; q++)
        if (!depth[q] || !grey[q]) return fail(SF_ERR_ARG, std::string(what) + ": null image");
    HIP_TRY(hipSetDevice(db->h->device));
    SfPlan p;
    const size_t o_frames = p.take((size_t)n * sizeof(KfFrame));
    if (int e = grow_scratch(db, p.off)) return e;
    return encode(db, FORM_DEVICE, n, nullptr, depth, grey, o_frames, 0, (uint32_t *)d_codes);
}

int sfk_query_streams(sfk_db *db, int n, const int32_t *streams, const int32_t *tags, int m, sfk_match *matches_out) {
    return query_or_add("sfk_query_streams", db, n, streams, nullptr, true, tags, m, matches_out, false, nullptr, nullptr, 0, nullptr);
}

int sfk_query_codes(sfk_db *db, int n, const uint32_t *codes, const int32_t *tags, int m, sfk_match *matches_out) {
    return query_or_add("sfk_query_codes", db, n, nullptr, codes, false, tags, m, matches_out, false, nullptr, nullptr, 0, nullptr);
}

int sfk_add_streams(sfk_db *db, int n, const int32_t *streams, const float *poses, const int32_t *tags, const int32_t *stamps, int min_distance,
                    int32_t *slots_out, sfk_match *nearest_out) {
    return query_or_add("sfk_add_streams", db, n, streams, nullptr, true, tags, 1, nearest_out, true, poses, stamps, min_distance, slots_out);
}

int sfk_add_codes(sfk_db *db, int n, const uint32_t *codes, const float *poses, const int32_t *tags, const int32_t *stamps, int min_distance,
                  int32_t *slots_out, sfk_match *nearest_out) {
    return query_or_add("sfk_add_codes", db, n, nullptr, codes, false, tags, 1, nearest_out, true, poses, stamps, min_distance, slots_out);
}

}  // extern "C"
