// The host-side resource owner (staticfusion_amd/csrc/sf_resources.h: SfOwner, its growth rule, SfRing), the per-call block
// of the companion interfaces (sf_call_block.h: SfPlan, SfCallBlock) and the lifetime of what is created from a handle
// (sf_parts.h: SfPart, SfParts) played through on the CPU. Stand-alone: the HIP functions the headers call are defined HERE --
// malloc-backed, with a set of live pointers (a free of an unknown one aborts), a log of calls and "fail the k-th acquiring call" --, and so is sf_fail. No HIP runtime, no
// library. tests/test_host_resources_cpu.py compiles it with -fsanitize=address,undefined and runs it as a child process: once
// without a failure, then once for every acquiring call of that run failing. It prints "ok <runs>" and returns 0, or names
// the first failure and returns 1. What is still allocated at exit is LeakSanitizer's to report.
#include <cstdio>
#include <cstdlib>
#include <map>

#include "../../staticfusion_amd/csrc/sf_parts.h"  // (includes sf_call_block.h, which includes sf_resources.h)

// ---- the HIP runtime of this program ---------------------------------------------------------------------------------
enum Op { MALLOC, FREE, HOST_MALLOC, HOST_FREE, EVENT_CREATE, EVENT_DESTROY, STREAM_CREATE, STREAM_DESTROY, STREAM_SYNC, EVENT_SYNC, EVENT_RECORD, MEMCPY, MEMSET, SET_DEVICE };
struct Call {
    Op op;
    const void *p;
};
static std::map<const void *, Op> live;  // pointer -> the call that made it
static std::vector<Call> calls;
struct Fill {  // a queued hipMemsetAsync
    const unsigned char *p;
    int value;
    size_t bytes;
};
static std::vector<Fill> fills;
static int acquired = 0;   // acquiring calls so far in this run
static int fail_at = 0;    // the acquiring call that fails (1-based), 0: none
static bool fired = false; // ... and it has
static Op failed_op = MALLOC;  // ... and which kind it was
static std::string last_error;

int sf_fail(int code, const std::string &msg) {
    last_error = msg;
    return code;
}

static hipError_t acquire(Op op, void **out, size_t bytes) {
    if (++acquired == fail_at) {
        fired = true;
        failed_op = op;
        return op == MALLOC ? hipErrorOutOfMemory : hipErrorUnknown;
    }
    void *p = std::malloc(bytes ? bytes : 1);
    if (!p) std::abort();
    live[p] = op;
    calls.push_back({op, p});
    *out = p;
    return hipSuccess;
}
static hipError_t release(Op op, Op made_by, void *p) {
    const auto it = live.find(p);
    if (it == live.end() || it->second != made_by) {
        std::fprintf(stderr, "release (op %d) of a pointer that is not live or of another kind\n", (int)op);
        std::abort();
    }
    live.erase(it);
    calls.push_back({op, p});
    std::free(p);
    return hipSuccess;
}
static void must_be_live(const void *p, Op made_by) {
    const auto it = live.find(p);
    if (it == live.end() || it->second != made_by) {
        std::fprintf(stderr, "use of a pointer that is not live\n");
        std::abort();
    }
}
extern "C" {
hipError_t hipMalloc(void **p, size_t bytes) { return acquire(MALLOC, p, bytes); }
hipError_t hipFree(void *p) { return release(FREE, MALLOC, p); }
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned) { return acquire(HOST_MALLOC, p, bytes); }
hipError_t hipHostFree(void *p) { return release(HOST_FREE, HOST_MALLOC, p); }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { return acquire(EVENT_CREATE, (void **)e, 1); }
hipError_t hipEventDestroy(hipEvent_t e) { return release(EVENT_DESTROY, EVENT_CREATE, e); }
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { return acquire(STREAM_CREATE, (void **)s, 1); }
hipError_t hipStreamDestroy(hipStream_t s) { return release(STREAM_DESTROY, STREAM_CREATE, s); }
hipError_t hipMemset(void *p, int v, size_t bytes) {
    must_be_live(p, MALLOC);
    std::memset(p, v, bytes);
    calls.push_back({MEMSET, p});
    return hipSuccess;
}
hipError_t hipSetDevice(int) {
    calls.push_back({SET_DEVICE, nullptr});
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t s) {
    must_be_live(s, STREAM_CREATE);
    calls.push_back({STREAM_SYNC, s});
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t e) {
    must_be_live(e, EVENT_CREATE);
    calls.push_back({EVENT_SYNC, e});
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) {
    must_be_live(e, EVENT_CREATE);
    must_be_live(s, STREAM_CREATE);
    calls.push_back({EVENT_RECORD, e});
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind, hipStream_t s) {
    must_be_live(dst, MALLOC);
    must_be_live(s, STREAM_CREATE);
    std::memcpy(dst, src, bytes);
    calls.push_back({MEMCPY, dst});
    return hipSuccess;
}
hipError_t hipMemsetAsync(void *p, int v, size_t bytes, hipStream_t s) {  // (p may lie inside a block: the caller checks the range)
    must_be_live(s, STREAM_CREATE);
    std::memset(p, v, bytes);
    fills.push_back({(const unsigned char *)p, v, bytes});
    calls.push_back({MEMSET, p});
    return hipSuccess;
}
const char *hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : "unknown error"; }
}

// ---- the scenario ---------------------------------------------------------------------------------------------------
static long checks = 0;
#define CHECK(cond)                                                                             \
    do {                                                                                        \
        checks++;                                                                               \
        if (!(cond)) {                                                                          \
            std::printf("FAILED %s:%d (failing call %d): %s\n", __FILE__, __LINE__, fail_at, #cond); \
            return 1;                                                                           \
        }                                                                                       \
    } while (0)

// a handle in miniature: the members the product's groups, grown blocks and rings set
struct SF_INTERNAL Mini {  // (hidden like the types it holds)
    SfOwner own;
    hipStream_t stream = nullptr;
    int *in0 = nullptr, *in1 = nullptr, *in2 = nullptr, *in3 = nullptr;  // like input_alloc
    hipStream_t copy_stream = nullptr;                                  // like the set-up of sf_upload_current_async
    hipEvent_t copy_done = nullptr, compute_done = nullptr;
    float *up0 = nullptr, *up1 = nullptr;
    float *block = nullptr;
    size_t block_cap = 0;
    int *pin = nullptr;
    size_t pin_cap = 0;
    SfRing<4, false> lazy;
    SfRing<8, true> eager;
};
static int group_of_four(Mini &m) {
    if (m.in0) return SF_OK;
    SfOwner g;
    int *a = nullptr, *b = nullptr, *c = nullptr, *d = nullptr;
    if (int e = g.device(&a, 100)) return e;
    if (int e = g.device(&b, 100)) return e;
    if (int e = g.device(&c, 100)) return e;
    if (int e = g.device(&d, 300)) return e;
    m.own.adopt(g);
    m.in0 = a; m.in1 = b; m.in2 = c; m.in3 = d;
    return SF_OK;
}
static int group_of_upload(Mini &m) {
    if (m.copy_stream) return SF_OK;
    SfOwner g;
    hipStream_t st = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    float *a = nullptr, *b = nullptr;
    if (int e = g.stream(&st, hipStreamNonBlocking)) return e;
    if (int e = g.event(&e0, hipEventDisableTiming)) return e;
    if (int e = g.event(&e1, hipEventDisableTiming)) return e;
    if (int e = g.device(&a, 64)) return e;
    if (int e = g.device(&b, 64)) return e;
    m.own.adopt(g);
    m.copy_stream = st; m.copy_done = e0; m.compute_done = e1; m.up0 = a; m.up1 = b;
    return SF_OK;
}
static int call_local(bool leave_early) {  // like sf_microbench_copy: everything goes with the call, on every path
    SfOwner call;
    char *a = nullptr, *b = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (int e = call.device(&a, 4096, false)) return e;
    if (int e = call.device(&b, 4096, false)) return e;
    if (int e = call.event(&e0, hipEventDefault)) return e;
    if (leave_early) return SF_OK;
    if (int e = call.event(&e1, hipEventDefault)) return e;
    return SF_OK;
}

// ---- a companion call in miniature (sf_hip_join.hip's shape): lay out, grow, take the zeroed table, fill, upload, clear
struct Rec {
    int a, b;
    void *p;
};
static int zero_pieces, ones_pieces, rest_pieces;  // the layout of the next block_call, in pieces of `piece` bytes
static int block_call(Mini &m, SfCallBlock &blk, size_t n, size_t piece, SfPlan *plan_out) {
    SfPlan p;
    const size_t o_tab = p.take(n * sizeof(Rec));
    p.zeros_from_here();
    for (int q = 0; q < zero_pieces; q++) p.take(piece);
    p.ones_from_here();
    for (int q = 0; q < ones_pieces; q++) p.take(piece);
    p.rest_from_here();
    for (int q = 0; q < rest_pieces; q++) p.take(piece);
    *plan_out = p;
    if (int e = blk.grow(m.own, p.off, m.stream)) return e;
    Rec *tab = blk.zeroed<Rec>(n);
    for (size_t q = 0; q < n; q++)
        if (tab[q].a || tab[q].b || tab[q].p) return sf_fail(SF_ERR_STATE, "a table handed out zeroed is not zero");
    for (size_t q = 0; q < n; q++) tab[q] = Rec{(int)q + 1, -1, &blk};  // (every byte a later, smaller call must not see)
    if (int e = blk.upload(o_tab, tab, n * sizeof(Rec), m.stream)) return e;
    return p.clear(blk.dev, m.stream);
}

// One step. If the run's failing call fell into it: the documented code came back, `untouched` holds (what the step would
// have set is as it was), and the same step once more, now without a failure, succeeds.
template <class Step, class Untouched>
static int step(Step run, Untouched untouched) {
    const int before = acquired;
    const bool had_fired = fired;
    int r = run();
    if (fired && !had_fired) {
        // device memory: SF_ERR_NOMEM, "hipMalloc: <HIP's text>"; pinned memory, events, streams: SF_ERR_DEVICE and their call's name
        if (failed_op == MALLOC) CHECK(r == SF_ERR_NOMEM && last_error == "hipMalloc: out of memory");
        else CHECK(r == SF_ERR_DEVICE && last_error == std::string(failed_op == HOST_MALLOC ? "hipHostMalloc" : failed_op == EVENT_CREATE ? "hipEventCreate" : "hipStreamCreate") + ": unknown error");
        CHECK(acquired > before);
        CHECK(untouched());
        r = run();
    }
    CHECK(r == SF_OK);
    return 0;
}
static size_t count_op(size_t from, Op op, const void *p = nullptr) {
    size_t n = 0;
    for (size_t q = from; q < calls.size(); q++) n += calls[q].op == op && (!p || calls[q].p == p);
    return n;
}
static long find_op(size_t from, Op op, const void *p) {
    for (size_t q = from; q < calls.size(); q++)
        if (calls[q].op == op && calls[q].p == p) return (long)q;
    return -1;
}
template <class Ring>
static bool ring_consistent(const Ring &r, int n) {
    for (int q = 0; q < n; q++)
        if (r.made(q) ? !(r.host[q] && r.dev[q] && r.event[q]) : (r.host[q] || r.dev[q] || r.event[q])) return false;
    return true;
}

// ---- a handle and its parts in miniature (sf_parts.h). The handle has what part_destroy of sf_host.h reads; a part has two
// blocks and a call block under its own owner, like a keyframe database.
struct SF_INTERNAL sf_handle {
    int device = 0;
    hipStream_t stream = nullptr;
    SfOwner own;
    SfParts parts;
};
struct SF_INTERNAL MiniPart : SfPart {
    float *a = nullptr, *b = nullptr;
    SfCallBlock blk;
    int hooks = 0;
    bool hook_in_order = false;
    void shelled() override {  // (orphan_all: the owner has released, h is still set)
        hooks++;
        hook_in_order = own.dev.empty() && h != nullptr;
        a = b = nullptr;
        blk.forget();
    }
};
static int part_create(sf_handle &h, bool enter, MiniPart **out) {  // (enter false: a create call that fails after h is set)
    MiniPart *p = new MiniPart;
    int e = p->own.device(&p->a, 100);
    if (!e) e = p->own.device(&p->b, 50, false);
    if (e) {
        delete p;  // (its owner releases what it had)
        return e;
    }
    p->h = &h;
    if (enter) h.parts.enter(p);
    *out = p;
    return SF_OK;
}
static void part_destroy(SfPart *p) {  // as sf_host.h has it
    sf_handle *h = p->h;
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    h->parts.leave(p);
    p->own.release_all();
}
static bool is_shell(const MiniPart *p) { return !p->h && !p->a && !p->b && !p->blk.dev && !p->blk.bytes && p->own.dev.empty() && p->hooks == 1 && p->hook_in_order; }

static int parts_scenario() {
    sf_handle A, B;
    for (sf_handle *h : {&A, &B})
        if (step([&] { return h->stream ? SF_OK : h->own.stream(&h->stream, hipStreamDefault); }, [&] { return h->stream == nullptr; })) return 1;
    const size_t n_streams = live.size();

    // ---- five parts under their own owners, one with a call block that was outgrown once: the handle goes first
    MiniPart *p[5] = {};
    for (int q = 0; q < 5; q++) {
        const size_t n_live = live.size();
        if (step([&] { return p[q] ? SF_OK : part_create(A, true, &p[q]); }, [&] { return !p[q] && live.size() == n_live && A.parts.list.size() == (size_t)q; })) return 1;
        CHECK(p[q]->h == &A && A.parts.list.size() == (size_t)q + 1 && A.parts.list.back() == p[q] && live.size() == n_live + 2);
    }
    for (size_t need : {3000, 9000}) {
        unsigned char *const dev0 = p[2]->blk.dev;
        if (step([&] { return p[2]->blk.grow(p[2]->own, need, A.stream); }, [&] { return p[2]->blk.dev == dev0; })) return 1;
    }
    CHECK(live.size() == n_streams + 11 && A.own.dev.empty());  // nothing of a part is the handle's
    std::vector<const void *> blocks;
    for (const auto &kv : live)
        if (kv.second == MALLOC) blocks.push_back(kv.first);
    size_t mark = calls.size();
    A.parts.orphan_all();
    CHECK(live.size() == n_streams && A.parts.list.empty() && count_op(mark, FREE) == 11 && calls.size() == mark + 11);
    for (const void *b : blocks) CHECK(count_op(mark, FREE, b) == 1);
    for (int q = 0; q < 5; q++) CHECK(is_shell(p[q]));
    A.parts.orphan_all();  // (an empty list: nothing)
    CHECK(calls.size() == mark + 11);
    // ---- a shell destroyed afterwards touches no HIP function
    mark = calls.size();
    for (int q = 0; q < 5; q++) {
        part_destroy(p[q]);
        delete p[q];
    }
    CHECK(calls.size() == mark);

    // ---- the part goes first: leave, release; orphan_all then frees nothing twice and leaves it alone
    MiniPart *first = nullptr, *stays = nullptr;
    if (step([&] { return first ? SF_OK : part_create(A, true, &first); }, [&] { return !first && A.parts.list.empty(); })) return 1;
    if (step([&] { return stays ? SF_OK : part_create(A, true, &stays); }, [&] { return !stays && A.parts.list.size() == 1; })) return 1;
    const void *const fa = first->a, *const fb = first->b;
    mark = calls.size();
    part_destroy(first);
    CHECK(calls[mark].op == SET_DEVICE && calls[mark + 1].op == STREAM_SYNC && calls[mark + 1].p == A.stream);  // the handle's device, after its queued work
    CHECK(find_op(mark, FREE, fa) > (long)mark + 1 && count_op(mark, FREE) == 2 && A.parts.list.size() == 1 && A.parts.list[0] == stays);
    A.parts.orphan_all();
    CHECK(count_op(mark, FREE, fa) == 1 && count_op(mark, FREE, fb) == 1 && first->hooks == 0 && first->h == &A && is_shell(stays));
    delete first;
    delete stays;
    CHECK(live.size() == n_streams);

    // ---- leave of a part that was never entered is harmless; so is the destroy of one that has h set and was not entered
    MiniPart *entered = nullptr, *half = nullptr;
    if (step([&] { return entered ? SF_OK : part_create(A, true, &entered); }, [&] { return !entered && A.parts.list.empty(); })) return 1;
    if (step([&] { return half ? SF_OK : part_create(A, false, &half); }, [&] { return !half && A.parts.list.size() == 1; })) return 1;
    A.parts.leave(half);
    CHECK(A.parts.list.size() == 1 && A.parts.list[0] == entered && live.size() == n_streams + 4);
    part_destroy(half);
    delete half;
    CHECK(A.parts.list.size() == 1 && A.parts.list[0] == entered && live.size() == n_streams + 2);

    // ---- rebind: the part leaves A and enters B; orphaning A leaves it alone, orphaning B makes it a shell
    A.parts.leave(entered);
    B.parts.enter(entered);
    entered->h = &B;
    mark = calls.size();
    A.parts.orphan_all();
    CHECK(calls.size() == mark && entered->h == &B && entered->a && entered->hooks == 0 && live.size() == n_streams + 2);
    entered->a[99] = 1.f;  // (still memory)
    B.parts.orphan_all();
    CHECK(is_shell(entered) && B.parts.list.empty() && live.size() == n_streams);
    mark = calls.size();
    part_destroy(entered);
    delete entered;
    CHECK(calls.size() == mark);
    return 0;
}

static int scenario(int failing, int *acquiring_calls) {
    live.clear();
    calls.clear();
    acquired = 0;
    fail_at = failing;
    fired = false;
    {
        Mini m;
        // the handle's stream: everything below drains or copies on it
        if (step([&] { return m.stream ? SF_OK : m.own.stream(&m.stream, hipStreamDefault); }, [&] { return m.stream == nullptr && live.empty(); })) return 1;

        // ---- a group of four blocks
        size_t n_live = live.size();
        if (step([&] { return group_of_four(m); }, [&] { return !m.in0 && !m.in1 && !m.in2 && !m.in3 && live.size() == n_live && m.own.dev.empty(); })) return 1;
        CHECK(m.in0 && m.in1 && m.in2 && m.in3 && live.size() == n_live + 4 && m.own.dev.size() == 4);
        for (int q = 0; q < 300; q++) CHECK(m.in3[q] == 0);  // zero-filled
        CHECK(group_of_four(m) == SF_OK && live.size() == n_live + 4);  // made: nothing more

        // ---- a group of a stream, two events and two blocks
        n_live = live.size();
        if (step([&] { return group_of_upload(m); },
                 [&] { return !m.copy_stream && !m.copy_done && !m.compute_done && !m.up0 && !m.up1 && live.size() == n_live && m.own.streams.size() == 1; }))
            return 1;
        CHECK(m.copy_stream && m.copy_done && m.compute_done && m.up0 && m.up1 && live.size() == n_live + 5);

        // ---- a block grown three times, one of them a no-op; then once past the geometric step
        size_t mark = calls.size();
        if (step([&] { return m.own.grow(&m.block, &m.block_cap, 2000, m.stream); }, [&] { return !m.block && m.block_cap == 0; })) return 1;
        CHECK(m.block && m.block_cap == 2000);                   // the first request is exact
        CHECK(count_op(mark, STREAM_SYNC) == 0 && count_op(mark, FREE) == 0);  // nothing outgrown: no drain
        mark = calls.size();
        float *const first = m.block;
        CHECK(m.own.grow(&m.block, &m.block_cap, 1500, m.stream) == SF_OK);
        CHECK(m.block == first && m.block_cap == 2000 && calls.size() == mark);  // a no-op makes no call at all
        n_live = live.size();
        if (step([&] { return m.own.grow(&m.block, &m.block_cap, 2001, m.stream); }, [&] { return m.block == first && m.block_cap == 2000 && live.size() == n_live; })) return 1;
        CHECK(m.block != first && m.block_cap == 2000 + 1000 + 1024 && live.size() == n_live);
        {
            const long made = find_op(mark, MALLOC, m.block), drained = find_op(mark, STREAM_SYNC, m.stream), freed = find_op(mark, FREE, first);
            CHECK(made >= 0 && made < drained && drained < freed);  // allocate new, drain, free old
            CHECK(count_op(0, FREE, first) == 1);                    // ... exactly once
        }
        if (step([&] { return m.own.grow(&m.block, &m.block_cap, 10000, m.stream, false); }, [&] { return m.block_cap == 4024; })) return 1;
        CHECK(m.block_cap == 10000);

        // ---- a pinned block grown
        if (step([&] { return m.own.grow_pinned(&m.pin, &m.pin_cap, 5000, m.stream); }, [&] { return !m.pin && m.pin_cap == 0; })) return 1;
        int *const first_pin = m.pin;
        CHECK(first_pin && m.pin_cap == 5000 && live.at(first_pin) == HOST_MALLOC);
        mark = calls.size();
        if (step([&] { return m.own.grow_pinned(&m.pin, &m.pin_cap, 5001, m.stream); }, [&] { return m.pin == first_pin && m.pin_cap == 5000; })) return 1;
        CHECK(m.pin != first_pin && m.pin_cap == 5000 + 2500 + 1024);
        {
            const long drained = find_op(mark, STREAM_SYNC, m.stream), freed = find_op(mark, HOST_FREE, first_pin);
            CHECK(drained >= 0 && drained < freed && count_op(0, HOST_FREE, first_pin) == 1);
        }

        // ---- a ring whose slots are made as they are reached, ten uploads
        for (unsigned i = 0; i < 10; i++) {
            const unsigned slot = i % 4;
            const unsigned table[4] = {i, i * 3, i * 5, 0xabcdu};
            void *dev = nullptr;
            mark = calls.size();
            n_live = live.size();
            if (step([&] { return m.lazy.next(m.own, 64, m.stream, table, sizeof table, &dev); },
                     [&] { return !m.lazy.made(slot) && m.lazy.calls == i && live.size() == n_live && ring_consistent(m.lazy, 4); }))
                return 1;
            CHECK(m.lazy.calls == i + 1 && dev == m.lazy.dev[slot] && ring_consistent(m.lazy, 4));
            CHECK(std::memcmp(dev, table, sizeof table) == 0 && std::memcmp(m.lazy.host[slot], table, sizeof table) == 0);
            CHECK(live.size() == n_live + (i < 4 ? 3 : 0));  // a slot is made by the call that first reaches it, and only then
            for (unsigned q = 0; q < 4; q++) CHECK(m.lazy.made(q) == (q <= i));
            // waited for before its reuse -- and before the copy into it --, not before its first use
            const long waited = find_op(mark, EVENT_SYNC, m.lazy.event[slot]), copied = find_op(mark, MEMCPY, dev);
            CHECK(count_op(mark, EVENT_SYNC) == (i >= 4 ? 1u : 0u) && copied >= 0 && (i < 4 || (waited >= 0 && waited < copied)));
            mark = calls.size();
            CHECK(m.lazy.done(m.stream) == SF_OK);
            CHECK(calls.size() == mark + 1 && find_op(mark, EVENT_RECORD, m.lazy.event[slot]) == (long)mark);
        }

        // ---- a ring made at once, ten uploads
        for (unsigned i = 0; i < 10; i++) {
            const unsigned slot = i % 8;
            const int frames[3] = {(int)i, -1, 7};
            void *dev = nullptr;
            mark = calls.size();
            n_live = live.size();
            if (step([&] { return m.eager.next(m.own, sizeof frames, m.stream, frames, sizeof frames, &dev); },
                     [&] { return m.eager.calls == 0 && i == 0 && ring_consistent(m.eager, 8) && count_op(mark, MEMCPY) == 0; }))
                return 1;
            CHECK(m.eager.calls == i + 1 && dev == m.eager.dev[slot] && ring_consistent(m.eager, 8));
            CHECK(std::memcmp(dev, frames, sizeof frames) == 0);
            CHECK(live.size() == n_live + (i == 0 ? 24 : 0));  // all eight slots at the first call: no later call allocates
            for (unsigned q = 0; q < 8; q++) CHECK(m.eager.made(q));
            const long waited = find_op(mark, EVENT_SYNC, m.eager.event[slot]), copied = find_op(mark, MEMCPY, dev);
            CHECK(count_op(mark, EVENT_SYNC) == (i >= 8 ? 1u : 0u) && copied >= 0 && (i < 8 || (waited >= 0 && waited < copied)));
            CHECK(m.eager.done(m.stream) == SF_OK);
            CHECK(calls.back().op == EVENT_RECORD && calls.back().p == m.eager.event[slot]);
        }

        // ---- the layout rule: 256-byte aligned, monotonic, the next piece never inside the last one
        {
            SfPlan p;
            size_t last = 0, last_bytes = 0;
            const size_t sizes[] = {0, 1, 255, 256, 257, 48, 4096, 3, 0, 0, 1000001};
            for (size_t q = 0; q < sizeof sizes / sizeof sizes[0]; q++) {
                const size_t o = p.take(sizes[q]);
                CHECK(o % 256 == 0 && p.off % 256 == 0 && o >= last + last_bytes && p.off >= o + sizes[q] && p.off < o + sizes[q] + 256);
                last = o;
                last_bytes = sizes[q];
            }
        }
        // ---- a call block: a small call, a larger one that outgrows the block, the small one again; the cleared ranges with
        // an empty zero range, an empty ones range, an empty rest and none empty
        {
            SfCallBlock blk;
            SfPlan p;
            const int layouts[5][3] = {{2, 3, 1}, {0, 2, 1}, {2, 0, 1}, {2, 3, 0}, {0, 0, 0}};
            const size_t ns[3] = {3, 40, 3}, pieces[3] = {100, 5000, 100};
            for (int l = 0; l < 5; l++)
                for (int c = 0; c < 3; c++) {
                    zero_pieces = layouts[l][0]; ones_pieces = layouts[l][1]; rest_pieces = layouts[l][2];
                    unsigned char *const dev0 = blk.dev;
                    const size_t bytes0 = blk.bytes;
                    const std::vector<unsigned char> host0 = blk.host[0];
                    mark = calls.size();
                    const size_t fills0 = fills.size();
                    // (a failing acquisition: the pointer, the capacity and the host copy are what they were before the call)
                    if (step([&] { return block_call(m, blk, ns[c], pieces[c], &p); }, [&] { return blk.dev == dev0 && blk.bytes == bytes0 && blk.host[0] == host0; })) return 1;
                    CHECK(blk.bytes >= p.off && blk.host[0].size() == ns[c] * sizeof(Rec));
                    CHECK(std::memcmp(blk.dev, blk.host[0].data(), blk.host[0].size()) == 0);  // the table is at its offset, 0
                    if (blk.dev != dev0 && dev0) {  // outgrown: the new block, the drain, and only then the old one freed, once
                        const long made = find_op(mark, MALLOC, blk.dev), drained = find_op(mark, STREAM_SYNC, m.stream), freed = find_op(mark, FREE, dev0);
                        CHECK(made >= 0 && made < drained && drained < freed && count_op(mark, FREE) == 1);
                    } else {
                        CHECK(count_op(mark, FREE) == 0 && (dev0 == nullptr || count_op(mark, MALLOC) == 0));
                    }
                    // the two fills cover exactly what lies between the marks, the ones directly behind the zeros
                    CHECK(fills.size() == fills0 + 2);
                    const Fill &z = fills[fills0], &o = fills[fills0 + 1];
                    const size_t piece_room = (pieces[c] + 255) / 256 * 256;
                    CHECK(z.value == 0 && z.p == blk.dev + p.o_zero && z.bytes == zero_pieces * piece_room);
                    CHECK(o.value == 0xFF && o.p == z.p + z.bytes && o.bytes == ones_pieces * piece_room);
                    CHECK(p.o_zero == (ns[c] * sizeof(Rec) + 255) / 256 * 256 && p.o_rest == p.o_zero + z.bytes + o.bytes);
                    CHECK(p.off == p.o_rest + rest_pieces * piece_room && p.off <= blk.bytes);
                    for (size_t q = 0; q < z.bytes; q++) CHECK(z.p[q] == 0);
                    for (size_t q = 0; q < o.bytes; q++) CHECK(o.p[q] == 0xFF);
                }
            CHECK(blk.bytes >= 40 * sizeof(Rec) + 5 * 5120);  // it did grow past its first size
            // a second host copy is independent of the first; a resized table keeps what it held
            int *second = blk.resized<int>(4, 1);
            second[3] = 7;
            CHECK(blk.host[0].size() == 3 * sizeof(Rec) && blk.resized<int>(6, 1)[3] == 7 && blk.resized<int>(6, 1)[5] == 0);
            m.own.free_device(blk.dev);
            blk.forget();
            CHECK(!blk.dev && !blk.bytes);
        }

        // ---- an owner on the stack, left by an early return and by the last one
        n_live = live.size();
        if (step([&] { return call_local(true); }, [&] { return live.size() == n_live; })) return 1;
        CHECK(live.size() == n_live);
        if (step([&] { return call_local(false); }, [&] { return live.size() == n_live; })) return 1;
        CHECK(live.size() == n_live);

        // ---- one block back before the rest, then everything
        m.own.free_device(m.in2);
        m.in2 = nullptr;
        CHECK(live.size() == n_live - 1);
        m.own.release_all();
        CHECK(live.empty());
        CHECK(m.own.dev.empty() && m.own.pinned.empty() && m.own.events.empty() && m.own.streams.empty());
    }  // (the destructor of an owner that has released everything does nothing: a second free would abort above)
    CHECK(live.empty());
    if (parts_scenario()) return 1;  // (its two handles release their streams on the way out)
    CHECK(live.empty());
    CHECK(failing == 0 || fired);
    *acquiring_calls = acquired;
    return 0;
}

int main() {
    int n = 0, unused = 0;
    if (scenario(0, &n)) return 1;
    if (n < 40) {
        std::printf("FAILED: only %d acquiring calls in the clean run\n", n);
        return 1;
    }
    int runs = 1;
    for (int k = 1; k <= n; k++, runs++)
        if (scenario(k, &unused)) return 1;
    std::printf("ok %d\n", runs);
    return 0;
}
