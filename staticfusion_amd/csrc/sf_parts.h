// sf_parts.h — the lifetime of everything that is created from an sf_handle and may outlive it: surfel maps (sf_map),
// keyframe databases (sfk_db), region trackers (sft_tracker), deformation graphs (sfd_graph), closure builders (sfc_builder), carvers (sfe_carver), registrars (sfg_registrar).
// One base, SfPart, and one list in the handle, SfParts. Host only, no kernel, and nothing of the product beyond
// sf_call_block.h / sf_resources.h (tests/cpp/resources_host.cpp compiles it with g++ against HIP functions of its own);
// sf_handle is only named here. What needs the handle's members -- part_destroy, check_part -- is in sf_host.h.
//
// THE LIFETIME RULES, stated here for every part:
//   - A part's device memory belongs to the part's own owner (SfPart::own), never to the handle's. So whoever goes first,
//     every block is released exactly once, by the part's owner.
//   - The create call sets SfPart::h and enters the part into its handle's list once it is complete. From then on the part
//     is in exactly one list, that of the handle h names (sfm_map_rebind: leave the old one, enter the new one).
//   - The part goes first (part_destroy, sf_host.h): with its handle's device current and its handle's stream drained, it
//     leaves the list and releases its owner; then it is deleted. A part that has h set but was never entered (a create call
//     that failed half-way) goes the same way: leave() of an absent part does nothing.
//   - The handle goes first (sf_destroy): with its device current and its stream drained it calls orphan_all(), then
//     releases its own owner. orphan_all takes the parts in the order they were entered; for each it releases the owner,
//     then calls shelled(), then sets h to null; then the list is empty.
//   - What is left is a shell: no device memory, h null. Its destroy call touches no HIP function and deletes it. Every
//     other call answers SF_ERR_STATE through check_part, except what reads only host members that the shell still has
//     (sf_map_info), and sfm_map_rebind, which answers SF_ERR_ARG.
#pragma once
#include <algorithm>
#include <vector>

#include "sf_call_block.h"  // (includes sf_resources.h)

struct sf_handle;

struct SF_INTERNAL SfPart {
    sf_handle *h = nullptr;  // null: a shell, its handle went first
    SfOwner own;             // every device block of the part
    virtual ~SfPart() = default;
    // orphan_all has released `own`: forget the call block(s) and null the device pointers the part keeps
    virtual void shelled() {}
};

// the parts of one handle (sf_handle::parts)
struct SF_INTERNAL SfParts {
    std::vector<SfPart *> list;

    void enter(SfPart *p) { list.push_back(p); }
    void leave(SfPart *p) { list.erase(std::remove(list.begin(), list.end(), p), list.end()); }
    void orphan_all() {
        for (SfPart *p : list) {
            p->own.release_all();
            p->shelled();
            p->h = nullptr;
        }
        list.clear();
    }
};
