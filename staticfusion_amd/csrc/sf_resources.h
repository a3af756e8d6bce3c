// sf_resources.h — who owns what the host side acquires from HIP: device blocks, pinned blocks, events, streams. One type,
// SfOwner, holds them for a handle, a map or a single call and releases them; one rule, SfOwner::grow, makes a block
// larger; one type, SfRing, is the ring of small per-call tables that go to the device without a host synchronisation.
// Host only, no kernel: this header needs the HIP runtime API and nothing of the product (tests/cpp/resources_host.cpp
// compiles it with g++ against HIP functions of its own).
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/sf.h"

#ifndef SF_INTERNAL
#define SF_INTERNAL __attribute__((visibility("hidden")))
#endif

// the thread's last error text (sf_last_error); returns `code` (defined in sf_hip.hip)
SF_INTERNAL int sf_fail(int code, const std::string &msg);

static inline int sf_hip_fail(int code, const char *what, hipError_t e) { return sf_fail(code, std::string(what) + ": " + hipGetErrorString(e)); }

// Everything a handle, a map or one call has acquired. Acquire through it, and it is released with the owner: by
// release_all (sf_destroy, a map's release) or by the destructor (an owner on the stack, on every return path).
//
// A GROUP of resources that only make sense together is acquired into an owner on the stack and into local variables;
// when every acquisition has succeeded, adopt() hands them to the lasting owner and the caller assigns its members.
// A failure in between returns, the local owner releases what it had, and no member has changed: nothing is half-made.
struct SF_INTERNAL SfOwner {
    std::vector<void *> dev, pinned;
    std::vector<hipEvent_t> events;
    std::vector<hipStream_t> streams;

    SfOwner() = default;
    SfOwner(const SfOwner &) = delete;
    SfOwner &operator=(const SfOwner &) = delete;
    ~SfOwner() { release_all(); }

    // `count` elements of device memory (at least one), zero-filled unless told otherwise (a map's blocks stay unfilled)
    template <class T>
    int device(T **p, size_t count, bool zero_fill = true) {
        void *q = nullptr;
        const size_t bytes = (count ? count : 1) * sizeof(T);
        hipError_t e = hipMalloc(&q, bytes);
        if (e != hipSuccess) return sf_hip_fail(SF_ERR_NOMEM, "hipMalloc", e);
        if (zero_fill && (e = hipMemset(q, 0, bytes)) != hipSuccess) {
            (void)hipFree(q);
            return sf_hip_fail(SF_ERR_DEVICE, "hipMemset", e);
        }
        dev.push_back(q);
        *p = (T *)q;
        return SF_OK;
    }
    template <class T>
    int pinned_block(T **p, size_t count) {
        void *q = nullptr;
        const hipError_t e = hipHostMalloc(&q, (count ? count : 1) * sizeof(T), hipHostMallocDefault);
        if (e != hipSuccess) return sf_hip_fail(SF_ERR_DEVICE, "hipHostMalloc", e);
        pinned.push_back(q);
        *p = (T *)q;
        return SF_OK;
    }
    int event(hipEvent_t *out, unsigned flags) {
        hipEvent_t ev = nullptr;
        const hipError_t e = hipEventCreateWithFlags(&ev, flags);
        if (e != hipSuccess) return sf_hip_fail(SF_ERR_DEVICE, "hipEventCreate", e);
        events.push_back(ev);
        *out = ev;
        return SF_OK;
    }
    int stream(hipStream_t *out, unsigned flags) {
        hipStream_t st = nullptr;
        const hipError_t e = hipStreamCreateWithFlags(&st, flags);
        if (e != hipSuccess) return sf_hip_fail(SF_ERR_DEVICE, "hipStreamCreate", e);
        streams.push_back(st);
        *out = st;
        return SF_OK;
    }

    // one block back before its owner goes (a block of this owner, or null)
    void free_device(void *p) {
        const auto it = std::find(dev.begin(), dev.end(), p);
        if (it == dev.end()) return;
        dev.erase(it);
        (void)hipFree(p);
    }
    void free_pinned(void *p) {
        const auto it = std::find(pinned.begin(), pinned.end(), p);
        if (it == pinned.end()) return;
        pinned.erase(it);
        (void)hipHostFree(p);
    }
    // everything (the caller has drained what may still use it); streams last, what was recorded on them is gone by then
    void release_all() {
        for (void *p : dev) (void)hipFree(p);
        for (void *p : pinned) (void)hipHostFree(p);
        for (hipEvent_t e : events) (void)hipEventDestroy(e);
        for (hipStream_t s : streams) (void)hipStreamDestroy(s);
        dev.clear();
        pinned.clear();
        events.clear();
        streams.clear();
    }
    // a completed group: what `g` holds is this owner's from here on
    void adopt(SfOwner &g) {
        for (void *p : g.dev) dev.push_back(p);
        for (void *p : g.pinned) pinned.push_back(p);
        for (hipEvent_t e : g.events) events.push_back(e);
        for (hipStream_t s : g.streams) streams.push_back(s);
        g.dev.clear();
        g.pinned.clear();
        g.events.clear();
        g.streams.clear();
    }

    // THE growth rule. A block of at least `count` elements: geometric growth (a map that gains a few surfels every frame
    // must not allocate every frame), and the outgrown block is released -- after `drain` has run dry, so that nothing
    // queued still reads it -- instead of living on with its owner. Order: allocate the new block, drain, free the old one.
    // *p and *capacity change together and only on success. The contents do not move: every user fills its block anew.
    template <class T>
    int grow(T **p, size_t *capacity, size_t count, hipStream_t drain, bool zero_fill = true) {
        return grow_any<T, false>(p, capacity, count, drain, zero_fill);
    }
    template <class T>
    int grow_pinned(T **p, size_t *capacity, size_t count, hipStream_t drain) {
        return grow_any<T, true>(p, capacity, count, drain, false);
    }

private:
    template <class T, bool PINNED>
    int grow_any(T **p, size_t *capacity, size_t count, hipStream_t drain, bool zero_fill) {
        if (*capacity >= count) return SF_OK;
        const size_t want = std::max(count, *capacity + *capacity / 2 + 1024);
        T *fresh = nullptr;
        if (int e = PINNED ? pinned_block(&fresh, want) : device(&fresh, want, zero_fill)) return e;
        T *old = *p;
        if (old) {
            const hipError_t e = hipStreamSynchronize(drain);
            if (e != hipSuccess) {
                PINNED ? free_pinned(fresh) : free_device(fresh);
                return sf_hip_fail(SF_ERR_DEVICE, "hipStreamSynchronize(h->stream)", e);
            }
            PINNED ? free_pinned(old) : free_device(old);
        }
        *p = fresh;
        *capacity = want;
        return SF_OK;
    }
};

// The ring of the small per-call tables (frame numbers of sf_advance_sequences_device, segment tables of the sfm_* calls): N
// slots, each a pinned block, a device block and an event. A call copies its table into the next slot's pinned block and
// queues the copy to the device block on its HIP stream (next), launches what reads the table, and records the slot's event
// behind it (done). So calls queue up behind running kernels without a host synchronisation; the host waits only when the
// slot it is about to overwrite was used N calls ago and that call has not executed yet.
// EAGER: the first call makes all N slots (no allocation in any later call); otherwise each slot is made by the call that
// first uses it. Either way a slot is all-or-nothing (a group, above), and a call that fails leaves the ring where it was.
template <int N, bool EAGER>
struct SF_INTERNAL SfRing {
    void *host[N] = {}, *dev[N] = {};
    hipEvent_t event[N] = {};
    bool used[N] = {};
    unsigned calls = 0;

    bool made(unsigned slot) const { return event[slot] != nullptr; }
    int make(SfOwner &own, unsigned slot, size_t slot_bytes) {
        if (made(slot)) return SF_OK;
        SfOwner g;
        unsigned char *h = nullptr, *d = nullptr;
        hipEvent_t ev = nullptr;
        if (int e = g.device(&d, slot_bytes)) return e;
        if (int e = g.pinned_block(&h, slot_bytes)) return e;
        if (int e = g.event(&ev, hipEventDisableTiming)) return e;
        own.adopt(g);
        host[slot] = h;
        dev[slot] = d;
        event[slot] = ev;
        return SF_OK;
    }
    // `bytes` (<= slot_bytes) of `src` on their way to the device on `st`; *dev_out is where they will be
    int next(SfOwner &own, size_t slot_bytes, hipStream_t st, const void *src, size_t bytes, void **dev_out) {
        const unsigned slot = calls % N;
        for (unsigned q = EAGER ? 0 : slot; q < (EAGER ? (unsigned)N : slot + 1); q++)
            if (int e = make(own, q, slot_bytes)) return e;
        if (used[slot]) {
            const hipError_t e = hipEventSynchronize(event[slot]);  // N calls ago
            if (e != hipSuccess) return sf_hip_fail(SF_ERR_DEVICE, "hipEventSynchronize(ring slot)", e);
        }
        used[slot] = true;
        calls++;
        std::memcpy(host[slot], src, bytes);
        const hipError_t e = hipMemcpyAsync(dev[slot], host[slot], bytes, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return sf_hip_fail(SF_ERR_DEVICE, "hipMemcpyAsync(ring slot)", e);
        *dev_out = dev[slot];
        return SF_OK;
    }
    // after the launch that reads the table of the last next()
    int done(hipStream_t st) {
        const hipError_t e = hipEventRecord(event[(calls - 1) % N], st);
        if (e != hipSuccess) return sf_hip_fail(SF_ERR_DEVICE, "hipEventRecord(ring slot)", e);
        return SF_OK;
    }
};
