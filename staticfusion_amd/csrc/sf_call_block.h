// sf_call_block.h — what one call of a companion interface (sfv_*, sfs_*, sfk_*, sfr_*, sfa_*, sfj_*, sft_*, sfb_*, sfp_*, sfd_*, sfc_*, sfe_*, sfg_*)
// lays out, fills and sends to the device: one rule for where the pieces of a call lie in a block (SfPlan), one type for
// the block with the host copies its tables are filled from (SfCallBlock). Host only, no kernel, and nothing of the product
// beyond sf_resources.h (tests/cpp/resources_host.cpp compiles it with g++ against HIP functions of its own).
//
// THE LIFETIME RULES, stated here for every part:
//   - A block belongs to one part (a member of sf_handle, of a keyframe database, of a tracker, of a deformation graph, of a closure builder, of a carver, of a registrar). A call grows, fills and
//     reads its own part's block and leaves every other part's block alone, so the results a caller still holds from
//     another part (sfv_last_large_sprites, a device-form output) stay what they were.
//   - The block holds the host copies of the tables: a member outlives the asynchronous upload queued from it, which a local
//     of the call would not. A call takes its tables from the block (zeroed / resized) and sends them with upload().
//   - The order within a call is: lay out (SfPlan), grow, then touch the host copies. A call whose growth fails has changed
//     neither the block nor a host copy. The contents of a block do not survive a call: every call fills what it reads.
#pragma once
#include <cstddef>
#include <vector>

#include "sf_resources.h"

// Where the pieces of a call lie in its block: take() hands out consecutive pieces, each starting on a multiple of 256 bytes.
// A layout may have one range that is filled with zero bytes and, directly behind it, one that is filled with 0xFF bytes
// before the kernels run: the caller marks where the first begins (zeros_from_here), where the second begins
// (ones_from_here) and where what is not cleared begins (rest_from_here), each before it takes the first piece of that
// range, and clear() queues both fills.
struct SF_INTERNAL SfPlan {
    size_t off = 0;  // bytes laid out so far: what the block must hold
    size_t o_zero = 0, o_ones = 0, o_rest = 0;

    size_t take(size_t bytes) {
        const size_t o = off;
        off = (off + bytes + 255) & ~(size_t)255;
        return o;
    }
    void zeros_from_here() { o_zero = off; }
    void ones_from_here() { o_ones = off; }
    void rest_from_here() { o_rest = off; }
    int clear(unsigned char *base, hipStream_t st) const {
        hipError_t e = hipMemsetAsync(base + o_zero, 0, o_ones - o_zero, st);
        if (e != hipSuccess) return sf_hip_fail(SF_ERR_DEVICE, "hipMemsetAsync(base + o_zero, 0, o_ones - o_zero, h->stream)", e);
        e = hipMemsetAsync(base + o_ones, 0xFF, o_rest - o_ones, st);
        if (e != hipSuccess) return sf_hip_fail(SF_ERR_DEVICE, "hipMemsetAsync(base + o_ones, 0xFF, o_rest - o_ones, h->stream)", e);
        return SF_OK;
    }
};

// The block of one part: device memory grown on demand by THE growth rule (SfOwner::grow), and two host copies -- the parts
// that draw maps first (score, refinement) fill the view table into copy 0 and their own table into copy 1; a part with
// two small tables that go up separately (region motion: entries and pairs; tracks: entries and slots) uses them likewise.
struct SF_INTERNAL SfCallBlock {
    unsigned char *dev = nullptr;
    size_t bytes = 0;  // capacity of dev
    std::vector<unsigned char> host[2];

    // at least `need` bytes, under `own`; an outgrown block is freed after `drain` has run dry
    int grow(SfOwner &own, size_t need, hipStream_t drain) { return own.grow(&dev, &bytes, need, drain); }
    // n records of host copy `copy`, every byte zero
    template <class T>
    T *zeroed(size_t n, int copy = 0) {
        host[copy].assign(n * sizeof(T), 0);
        return (T *)host[copy].data();
    }
    // n records of host copy `copy`; what the last call left in them stays (for a table whose every field the call sets)
    template <class T>
    T *resized(size_t n, int copy = 0) {
        host[copy].resize(n * sizeof(T));
        return (T *)host[copy].data();
    }
    // `count` bytes at `src` (inside a host copy) on their way to offset `offset` of the block on `st`
    int upload(size_t offset, const void *src, size_t count, hipStream_t st) {
        const hipError_t e = hipMemcpyAsync(dev + offset, src, count, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return sf_hip_fail(SF_ERR_DEVICE, "hipMemcpyAsync(call block table)", e);
        return SF_OK;
    }
    // the owner has released the memory (sf_destroy of the handle): an empty shell
    void forget() {
        dev = nullptr;
        bytes = 0;
    }
};
