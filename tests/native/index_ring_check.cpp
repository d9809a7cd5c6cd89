// Host check of csrc/index_ring.h (tests/test_index_ring_cpu.py compiles and runs it, with -fsanitize=address,undefined and
// plainly): where the sampled training loop keeps an iteration's indices and batch size (IndexRingLayout), which chunks are on
// the device and which host slots go back to the samplers (UploadWindow, driven by a fake event query), and where the iteration
// after a given one lives (successor).
#include "index_ring.h"

#include <cstdio>
#include <set>
#include <vector>

using gnn::host::ChunkSchedule;
using gnn::host::IndexRingLayout;
using gnn::host::kIndexChunkCap;
using gnn::host::kIndexPinnedBound;
using gnn::host::kIndexRingSlots;
using gnn::host::RingPos;
using gnn::host::UploadPoll;
using gnn::host::UploadWindow;

static int g_failed = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); g_failed++; } \
    } while (0)

static void check_layout(int members, int batch, int cap) {
    const IndexRingLayout lay{members, cap, batch};
    CHECK(lay.slot_elems() == (size_t)cap * batch);
    CHECK(lay.slice_elems() % 64 == 0 && lay.slice_elems() >= lay.slot_elems() * lay.slots && lay.slice_elems() < lay.slot_elems() * lay.slots + 64);
    CHECK(lay.total_elems() == lay.slice_elems() * members && lay.total_counts() == lay.count_slice() * members);
    std::set<size_t> idx, cnt;
    size_t n = 0;
    for (int m = 0; m < members; m++)
        for (int c = 0; c < lay.slots; c++)
            for (int at = 0; at < cap; at++, n++) {
                const size_t i = lay.index_at(m, c, at), k = lay.count_at(m, c, at);
                idx.insert(i); cnt.insert(k);
                // inside member m's slice, a whole batch of it, and no batch runs into the next iteration's
                CHECK(i >= (size_t)m * lay.slice_elems() && i + batch <= (size_t)(m + 1) * lay.slice_elems());
                CHECK(k >= (size_t)m * lay.count_slice() && k < (size_t)(m + 1) * lay.count_slice());
                CHECK(i % batch == ((size_t)m * lay.slice_elems()) % batch); // (batches tile the slice: two distinct offsets are a batch apart)
                // the pointer rule of the index region: member m's address is member 0's + m slices
                CHECK(i == lay.index_at(0, c, at) + (size_t)m * lay.slice_elems());
                CHECK(k == lay.count_at(0, c, at) + (size_t)m * lay.count_slice());
                // chunk c + slots shares the slot, chunk c + 1 does not
                CHECK(lay.index_at(m, c + lay.slots, at) == i && lay.count_at(m, c + lay.slots, at) == k);
                CHECK(lay.index_at(m, c + 1, at) != i && lay.count_at(m, c + 1, at) != k);
            }
    CHECK(idx.size() == n && cnt.size() == n); // injective over (member, slot, position)
    CHECK(*idx.rbegin() + batch <= lay.total_elems() && *cnt.rbegin() < lay.total_counts());
    for (int m = 0; m < members; m++) CHECK(lay.index_at(m, 0, 0) % 64 == 0); // a slice starts on a 256-byte boundary
    CHECK(lay.slot(0) == lay.slot(4) && lay.slot(4) == 0 && lay.slot(7) == 3 && lay.slot(3) != lay.slot(4));
}

static void check_chunk_cap() {
    // one ring is never shortened, whatever the batch
    CHECK(IndexRingLayout::chunk_cap(1, 1) == 256 && IndexRingLayout::chunk_cap(1, 4096) == 256 && IndexRingLayout::chunk_cap(1, 1 << 20) == 256);
    // n rings: halved from 256 while they exceed 64 MiB together
    CHECK(kIndexRingSlots == 4 && kIndexChunkCap == 256 && kIndexPinnedBound == ((size_t)64 << 20));
    CHECK(IndexRingLayout::chunk_cap(16, 128) == 256 && IndexRingLayout::chunk_cap(3, 48) == 256);
    CHECK(IndexRingLayout::chunk_cap(16, 1024) == 256);  // 16 * 4 * 256 * 1024 * 4 = 64 MiB exactly: within the bound
    CHECK(IndexRingLayout::chunk_cap(16, 1025) == 128);
    const int cap = IndexRingLayout::chunk_cap(16, 4096);
    CHECK(cap == 64 && (size_t)16 * 4 * cap * 4096 * 4 <= kIndexPinnedBound && (size_t)16 * 4 * (2 * cap) * 4096 * 4 > kIndexPinnedBound);
    CHECK(IndexRingLayout::chunk_cap(2, 1 << 24) == 1); // never below one iteration
    const IndexRingLayout lay{16, cap, 4096};
    CHECK(lay.members == 16 && lay.slots == 4 && lay.cap == 64 && lay.batch == 4096 && lay.total_elems() * 4 <= kIndexPinnedBound);
}

// A fake device: event of chunk c completes at time done_at[c]; an event may be broken.  Records what the window asked.
struct FakeEvents {
    std::vector<int> done_at;
    int now = 0, broken = -1;
    std::vector<int> waited, handed; // chunks the window blocked on; the `upto` of every hand-back
    UploadPoll poll(int c, bool wait) {
        if (c == broken) return UploadPoll::error;
        if (wait) { waited.push_back(c); now = std::max(now, done_at[(size_t)c]); }
        return done_at[(size_t)c] <= now ? UploadPoll::done : UploadPoll::not_ready;
    }
};

static bool release(UploadWindow &w, FakeEvents &ev, bool wait) {
    const int before = w.released;
    const size_t calls = ev.handed.size();
    const bool ok = w.release(wait, [&](int c, bool block) { return ev.poll(c, block); }, [&](int upto) { ev.handed.push_back(upto); });
    // hand_back exactly when `released` advances, with the new value; every chunk handed back has completed
    CHECK((w.released != before) == (ev.handed.size() == calls + 1) && ev.handed.size() <= calls + 1);
    if (w.released != before) CHECK(ev.handed.back() == w.released);
    for (int c = before; c < w.released; c++) CHECK(ev.done_at[(size_t)c] <= ev.now);
    CHECK(w.released >= before && w.released <= w.uploaded && w.uploaded <= w.released + w.slots);
    if (!ok) CHECK(w.released == before);
    return ok;
}

// The loop's own sequence (sampler.hip: stage) over `chunks` chunks: release what is done, upload chunk c if it is the next one --
// blocking on the oldest upload while every slot is taken --, then chunk c + 1 ahead when `ahead`.  Time advances by one per chunk.
static void drive(int chunks, bool ahead, int lag, int burst_every) {
    UploadWindow w;
    w.sched = ChunkSchedule{chunks * 4, 4};
    FakeEvents ev;
    for (int c = 0; c < chunks; c++) ev.done_at.push_back(burst_every ? (c / burst_every + 1) * burst_every + lag : c + lag); // (bursts: several complete at once)
    for (int c = 0; c < chunks; c++, ev.now++) {
        CHECK(release(w, ev, false));
        CHECK(w.next(c) || w.uploaded == c + 1);
        for (int u = c; u <= c + (ahead ? 1 : 0) && u < chunks; u++) {
            if (!w.next(u)) continue;
            if (u > c && w.full()) continue; // (the chunk ahead is not drawn -- its host slot is not the samplers' yet -- and the loop never waits for it)
            if (w.full()) { // the samplers cannot draw chunk c: its host slot is chunk c - slots's, not yet handed back
                const size_t n_waits = ev.waited.size();
                CHECK(release(w, ev, true));
                CHECK(ev.waited.size() == n_waits + 1 && ev.waited.back() == u - w.slots); // the OLDEST one, once
                CHECK(!w.full());
            }
            CHECK(u < w.released + w.slots); // its host slot has been handed back: the samplers could draw it
            w.uploaded_chunk(u);
            CHECK(w.uploaded == u + 1);
        }
    }
    ev.now += chunks + lag + burst_every;
    CHECK(release(w, ev, false) && w.released == chunks && w.uploaded == chunks);
    for (size_t i = 1; i < ev.handed.size(); i++) CHECK(ev.handed[i] > ev.handed[i - 1]);
}

static void check_window() {
    for (int ahead = 0; ahead < 2; ahead++) {
        drive(23, ahead != 0, 0, 0);  // every event done by the next look
        drive(23, ahead != 0, 2, 0);  // late, one by one
        drive(23, ahead != 0, 9, 0);  // so late that all four slots are taken: the loop blocks on the oldest
        drive(23, ahead != 0, 1, 3);  // several at once
        drive(23, ahead != 0, 7, 5);
        drive(1, ahead != 0, 3, 0);
    }
    { // an error from poll: reported, nothing handed back, not even the chunks in front of the broken one
        UploadWindow w;
        FakeEvents ev;
        ev.done_at = {0, 0, 0, 0};
        ev.broken = 2;
        for (int c = 0; c < 4; c++) w.uploaded_chunk(c);
        CHECK(w.full());
        CHECK(!release(w, ev, false) && w.released == 0 && ev.handed.empty());
        CHECK(!release(w, ev, true) && w.released == 0 && ev.waited == std::vector<int>{0}); // (the wait itself was for the oldest)
        ev.broken = -1;
        CHECK(release(w, ev, false) && w.released == 4 && ev.handed == std::vector<int>{4} && !w.full());
    }
    { // not ready stops at the first unfinished upload, later finished ones stay; waiting applies to the oldest only
        UploadWindow w;
        FakeEvents ev;
        ev.done_at = {0, 5, 0, 9};
        for (int c = 0; c < 4; c++) w.uploaded_chunk(c);
        CHECK(release(w, ev, false) && w.released == 1 && !w.full());
        CHECK(release(w, ev, false) && w.released == 1 && ev.handed.size() == 1); // nothing new: no hand-back
        CHECK(release(w, ev, true) && w.released == 3 && ev.waited == std::vector<int>{1} && ev.now == 5); // chunk 3 is not waited for
        CHECK(w.next(4) && !w.next(3) && !w.next(5));
    }
}

static void check_successor() {
    UploadWindow w;
    w.sched = ChunkSchedule{260, 256}; // chunks begin at 0, 16, 48, 112, 240; the last one holds 20 iterations
    CHECK(w.sched.chunks() == 5 && w.sched.length(0) == 16 && w.sched.length(4) == 20);
    w.uploaded_chunk(0);
    RingPos p = w.successor(0, 3);
    CHECK(p && p.chunk == 0 && p.at == 4);                       // inside a chunk
    p = w.successor(0, 14);
    CHECK(p && p.chunk == 0 && p.at == 15);
    CHECK(!w.successor(0, 15));                                  // a chunk's last iteration, the next chunk not uploaded
    w.uploaded_chunk(1);
    p = w.successor(0, 15);
    CHECK(p && p.chunk == 1 && p.at == 0);                       // ... and uploaded
    CHECK(!w.successor(1, 31));
    for (int c = 2; c < 5; c++) w.uploaded_chunk(c);
    p = w.successor(3, 127);
    CHECK(p && p.chunk == 4 && p.at == 0);
    p = w.successor(4, 18);
    CHECK(p && p.chunk == 4 && p.at == 19);
    CHECK(!w.successor(4, 19));                                  // the run's last iteration
    // every iteration of a fully uploaded run has its successor at the next iteration number
    int i = 0;
    for (RingPos q{0, 0}; q; q = w.successor(q.chunk, q.at), i++) CHECK(w.sched.begin(q.chunk) + q.at == i);
    CHECK(i == 260);
    UploadWindow one;
    one.sched = ChunkSchedule{1, 256};
    one.uploaded_chunk(0);
    CHECK(!one.successor(0, 0));
}

int main() {
    const int members[] = {1, 3, 16}, batches[] = {1, 27, 128}, caps[] = {256, 8};
    for (int m : members) for (int b : batches) for (int cap : caps) check_layout(m, b, cap);
    check_chunk_cap();
    check_window();
    check_successor();
    if (g_failed) { std::printf("%d checks failed\n", g_failed); return 1; }
    std::printf("index ring ok\n");
    return 0;
}
