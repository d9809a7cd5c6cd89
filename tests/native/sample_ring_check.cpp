// Host check of csrc/sample_ring.h (tests/test_sample_ring_cpu.py compiles and runs it, with -fsanitize=thread and plainly):
// K producers' parts of every chunk against one consumer, a ring of 4 slots and short chunks.  Every chunk must be handed
// over once, in order, only after ALL members' parts of it are drawn, a slot must not be redrawn before it is released, an
// error raised in the middle and an early stop must end every thread.
#include "sample_ring.h"

#include <atomic>
#include <cstdio>
#include <vector>

using gnn::host::ChunkSchedule;
using gnn::host::SampleRing;
using gnn::host::SampleWorkers;

static int g_failed = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); g_failed++; } \
    } while (0)

static constexpr int kSlots = 4;

// One run: K members, `chunks` chunks of `len` values; fail_at >= 0: member fail_member's draw of that chunk fails;
// stop_after >= 0: the consumer leaves after that many chunks.  Returns the chunks the consumer took.
static int run(int K, int chunks, int len, int fail_at, int fail_member, int stop_after, int *rc_out) {
    // slot contents: value = chunk * 1000 + member * 10 + position, so that a slot overwritten too early or read too early shows
    std::vector<int> data((size_t)K * kSlots * len, -1);
    std::atomic<int> live_threads{0}, draws{0};
    int taken = 0;
    *rc_out = 0;
    SampleRing ring(K, kSlots, chunks);
    {
        SampleWorkers workers(ring, SampleWorkers::threads_for(K), [&](int m, int c, std::string *msg) -> int {
            struct Live { std::atomic<int> &n; Live(std::atomic<int> &n_) : n(n_) { n++; } ~Live() { n--; } } live(live_threads);
            if (c == fail_at && m == fail_member) { *msg = "drawing failed"; return 7; }
            int *slot = data.data() + ((size_t)m * kSlots + c % kSlots) * len;
            for (int i = 0; i < len; i++) slot[i] = c * 1000 + m * 10 + i;
            draws++;
            return 0;
        });
        for (int c = 0; c < chunks; c++) {
            if (c == stop_after) break;
            while (!ring.wait_ready(c, 200)) {}
            std::string msg;
            if (const int rc = ring.error(&msg)) { *rc_out = rc; CHECK(msg == "drawing failed"); break; }
            CHECK(ring.ready(c));
            for (int m = 0; m < K; m++) { // every member's part is there, and it is chunk c's (not c + kSlots's, not c - kSlots's)
                const int *slot = data.data() + ((size_t)m * kSlots + c % kSlots) * len;
                for (int i = 0; i < len; i++) CHECK(slot[i] == c * 1000 + m * 10 + i);
            }
            taken++;
            // (slots go back late and several at a time, as upload events complete)
            if (c % 3 == 2 || c + 1 == chunks) ring.release(c + 1);
        }
    } // ~SampleWorkers: stop + join
    CHECK(live_threads.load() == 0);
    if (fail_at < 0 && stop_after < 0) CHECK(draws.load() == K * chunks);
    CHECK(draws.load() <= K * std::min(chunks, taken + kSlots)); // no producer ran further ahead than the ring allows
    return taken;
}

int main() {
    { // the chunk schedule: 16, 32, 64, 128, then 256 each; a short cap; every iteration in exactly one chunk
        const ChunkSchedule s{1000, 256};
        const int want[] = {0, 16, 48, 112, 240, 496, 752, 1008};
        for (int c = 0; c < 8; c++) CHECK(s.begin(c) == want[c]);
        CHECK(s.chunks() == 7 && s.end(6) == 1000 && s.end(0) == 16);
        const ChunkSchedule t{50, 4};
        CHECK(t.begin(0) == 0 && t.begin(1) == 4 && t.begin(5) == 20 && t.chunks() == 13 && t.end(12) == 50);
        const ChunkSchedule u{13, 256};
        CHECK(u.chunks() == 1 && u.end(0) == 13);
        const ChunkSchedule v{40, 32};
        CHECK(v.begin(1) == 16 && v.begin(2) == 48 && v.chunks() == 2 && v.end(1) == 40);
    }
    CHECK(SampleWorkers::threads_for(1) == 1 && SampleWorkers::threads_for(3) == 3 && SampleWorkers::threads_for(16) == 8);
    const int Ks[] = {1, 3, 16};
    for (int K : Ks) {
        int rc = 0;
        CHECK(run(K, 23, 5, -1, 0, -1, &rc) == 23 && rc == 0);              // the whole run
        CHECK(run(K, 23, 5, 9, K - 1, -1, &rc) <= 9 && rc == 7);            // a producer error in the middle: reported, every thread ends
        CHECK(run(K, 23, 5, 0, 0, -1, &rc) == 0 && rc == 7);                // ... in the very first part
        CHECK(run(K, 23, 5, -1, 0, 6, &rc) == 6 && rc == 0);                // the consumer stops early: the producers wait for slots, then end
        CHECK(run(K, 2, 1, -1, 0, 0, &rc) == 0 && rc == 0);                 // ... before it took anything
    }
    if (g_failed) { std::printf("%d checks failed\n", g_failed); return 1; }
    std::printf("sample ring ok\n");
    return 0;
}
