// index_ring.h -- internal: the arithmetic of the sampled training loop's index storage (sampler.hip).  The run is cut into chunks
// (sample_ring.h: ChunkSchedule); chunk c of member m lives in slot c % slots of ring m, on the host (pinned) and on the
// device, and the rings are the slices of ONE allocation on either side.  Here: where an iteration's indices and its batch
// size lie (IndexRingLayout), which chunks are on the device and which host slots may go back to the samplers
// (UploadWindow), and where the iteration after a given one is to be found.  Plain C++, no HIP, no thread: sampler.hip binds
// the event query to hipEventQuery / hipEventSynchronize, tests/native/index_ring_check.cpp to its own.
#pragma once
#include "sample_ring.h"

#include <cstddef>
#include <cstdint>

namespace gnn {
namespace host {

constexpr int kIndexRingSlots = 4, kIndexChunkCap = 256;
constexpr size_t kIndexPinnedBound = (size_t)64 << 20; // all rings of a call together, pinned

// The ONE place where an offset into index or count storage is computed: host ring, device ring and both count arrays (the
// samplers' and the copy made at upload) are laid out alike.  `batch` is the largest nominal batch size of the call: the
// stride of every ring, so that member m's index pointer is member 0's + m * slice_elems() (group_kernels.h's index region).
struct IndexRingLayout {
    static constexpr int slots = kIndexRingSlots; // (a constant: c % slots is a mask in the step loop)
    int members = 1, cap = kIndexChunkCap, batch = 1;
    // iterations per chunk at most: for n > 1 rings halved from kIndexChunkCap until the n rings fit the pinned bound
    static int chunk_cap(int members, int batch) {
        int cap = kIndexChunkCap;
        if (members > 1) while (cap > 1 && (size_t)members * kIndexRingSlots * cap * batch * sizeof(int32_t) > kIndexPinnedBound) cap /= 2;
        return cap;
    }
    int slot(int chunk) const { return chunk % slots; }
    size_t slot_elems() const { return (size_t)cap * batch; }
    size_t slice_elems() const { return (slot_elems() * slots + 63) / 64 * 64; } // (a slice starts on a 256-byte boundary)
    size_t total_elems() const { return slice_elems() * members; }
    size_t count_slice() const { return (size_t)cap * slots; }
    size_t total_counts() const { return count_slice() * members; }
    // member m, chunk `chunk`, iteration `at` of that chunk: its first index / its batch size
    size_t index_at(int m, int chunk, int at) const { return (size_t)m * slice_elems() + (size_t)slot(chunk) * slot_elems() + (size_t)at * batch; }
    size_t count_at(int m, int chunk, int at) const { return (size_t)m * count_slice() + (size_t)slot(chunk) * cap + at; }
};

// an iteration as (chunk, position in the chunk); chunk < 0: none
struct RingPos { int chunk = -1, at = 0; explicit operator bool() const { return chunk >= 0; } };

enum class UploadPoll { done, not_ready, error };

// Chunks [0, uploaded) have their draws on the device (or in flight in front of every launch that reads them); the host slots
// of chunks [0, released) are the samplers' again, their upload's event having completed.  released <= uploaded <= released + slots.
struct UploadWindow {
    static constexpr int slots = kIndexRingSlots;
    ChunkSchedule sched;
    int uploaded = 0, released = 0;
    bool next(int c) const { return c == uploaded; }           // chunk c is the next to upload
    bool full() const { return uploaded - released >= slots; } // every slot taken and none released: wait for the oldest upload
    void uploaded_chunk(int c) { uploaded = c + 1; }
    // Hands finished uploads' host slots back, oldest first, up to the first one whose event has not completed.
    // poll(chunk, wait) -> UploadPoll asks for chunk's event; wait (wait_oldest, and only for the OLDEST chunk not yet released):
    // block until it has completed.  hand_back(upto), called exactly when `released` advances: the slots of chunks [0, upto) are
    // free.  false: poll reported an error (nothing is handed back).
    template <class Poll, class HandBack> bool release(bool wait_oldest, Poll poll, HandBack hand_back) {
        int r = released;
        for (; r < uploaded; r++) {
            const UploadPoll q = poll(r, wait_oldest && r == released);
            if (q == UploadPoll::error) return false;
            if (q == UploadPoll::not_ready) break;
        }
        if (r != released) { released = r; hand_back(r); }
        return true;
    }
    // where the iteration after (chunk, at) lives: the same chunk, or position 0 of the next one when that is uploaded; none
    // when it is not on the device yet (or the run ends here)
    RingPos successor(int chunk, int at) const {
        if (at + 1 < sched.length(chunk)) return RingPos{chunk, at + 1};
        return uploaded > chunk + 1 ? RingPos{chunk + 1, 0} : RingPos{};
    }
};

} // namespace host
} // namespace gnn
