// Host check of csrc/lookahead.h (tests/test_lookahead_cpu.py compiles and runs it): every transition of the two-launch
// step's look-ahead state writes exactly its set of fields, and member 0's state rebased to member k equals what member k
// holds after the same transitions on its own buffers.  "Leaves the rest alone" is checked field by field and with
// operator==, which compares every field.
#include "../../graph-neural-net_amd/csrc/lookahead.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using gnn::host::Lookahead;
using gnn::host::NextBatch;

static int g_failed = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); g_failed++; } \
    } while (0)

// a state with everything set: slabs of `s` with a staged copy (xstage_cur 1), `n` announced
static Lookahead full(const NextBatch &s, const NextBatch &n) {
    Lookahead a;
    a.slabs_now_hold(s, true);
    a.announce(n);
    return a;
}

int main() {
    std::vector<float> dataset(64), other(64);       // shared by every member: outside the arena
    std::vector<int32_t> ring(32);
    const size_t S = 256;
    std::vector<char> arena(3 * S);                  // three members' slices
    const float *dx = dataset.data();
    const NextBatch b0{dx, nullptr, 6}, b1{dx + 16, nullptr, 6}, s0{dx, ring.data(), 6}, s1{dx, ring.data() + 8, 6};

    { // a fresh state holds nothing
        Lookahead a;
        CHECK(!a.slabs_hold(b0) && !a.have_next && !a.xstage_valid && a.xstage_cur == 0);
        CHECK(a == Lookahead());
    }
    { // take_next is good once, and touches the announcement only
        Lookahead a = full(s0, s1), before = a;
        NextBatch nb{};
        CHECK(a.take_next(&nb) && nb == s1);
        CHECK(!a.have_next && a.slabs_hold(s0) && a.xstage_valid && a.xstage_cur == 1);
        NextBatch again{other.data(), nullptr, 1};
        CHECK(!a.take_next(&again) && again.a0 == other.data() && again.B == 1);
        a.announce(s1);
        CHECK(a == before);
    }
    { // slabs_hold distinguishes address, index vector and size
        Lookahead a;
        a.slabs_now_hold(s0, false);
        CHECK(a.slabs_hold(s0));
        CHECK(!a.slabs_hold(NextBatch{dx + 16, ring.data(), 6}));
        CHECK(!a.slabs_hold(NextBatch{dx, nullptr, 6}) && !a.slabs_hold(s1));
        CHECK(!a.slabs_hold(NextBatch{dx, ring.data(), 5}));
    }
    { // slabs_now_hold toggles xstage_cur only with a staged copy, and leaves the announcement alone
        Lookahead a;
        a.announce(b1);
        a.slabs_now_hold(b0, false);
        CHECK(a.slabs_hold(b0) && a.xstage_cur == 0 && !a.xstage_valid && a.have_next && a.next == b1);
        a.slabs_now_hold(s0, true);
        CHECK(a.slabs_hold(s0) && !a.slabs_hold(b0) && a.xstage_cur == 1 && a.xstage_valid);
        a.slabs_now_hold(s1, true);
        CHECK(a.xstage_cur == 0 && a.xstage_valid);
        a.slabs_now_hold(b0, false);
        CHECK(a.xstage_cur == 0 && !a.xstage_valid && a.have_next);
    }
    { // the chain step's own transitions
        Lookahead a = full(s0, s1);
        a.step_takes_slabs();
        CHECK(!a.slabs_hold(s0) && a.have_next && a.next == s1 && a.xstage_valid && a.xstage_cur == 1);
        a.step_left_no_slabs();
        CHECK(!a.slabs_hold(s0) && a.have_next && !a.xstage_valid && a.xstage_cur == 1);
        a.step_kept_weights(s0, true);
        CHECK(a == full(s0, s1));                     // (valid again, the buffer not toggled)
        a.step_kept_weights(b0, false);
        CHECK(a.slabs_hold(b0) && !a.xstage_valid && a.xstage_cur == 1 && a.have_next);
    }
    { // each clear writes exactly its set
        const Lookahead start = full(s0, s1);
        Lookahead a = start;
        a.weights_replaced();
        CHECK(!a.slabs_hold(s0) && a.have_next && a.next == s1 && a.xstage_valid && a.xstage_cur == 1);
        a.step_kept_weights(s0, true);
        CHECK(a == start);
        a.hint_unused();
        CHECK(a.slabs_hold(s0) && !a.have_next && a.xstage_valid && a.xstage_cur == 1);
        a.announce(s1);
        CHECK(a == start);
        a.slabs_of_staging_buffer();
        CHECK(!a.slabs_hold(s0) && a.have_next && !a.xstage_valid && a.xstage_cur == 1);
        a.step_kept_weights(s0, true);
        CHECK(a == start);
        a.rows_renamed();
        CHECK(!a.slabs_hold(s0) && !a.have_next && a.xstage_valid && a.xstage_cur == 1);
        a.step_kept_weights(s0, true); a.announce(s1);
        CHECK(a == start);
        a.forget();
        CHECK(!a.slabs_hold(s0) && !a.have_next && !a.xstage_valid && a.xstage_cur == 1);
        a.step_kept_weights(s0, true); a.announce(s1);
        CHECK(a == start);
    }
    { // rebased moves pointers inside [lo, lo + S) and leaves dataset and ring pointers (and null) alone
        const char *lo = arena.data();
        const float *stage0 = reinterpret_cast<const float *>(lo + 64);         // member 0's host-batch A_0 buffer
        const int32_t *idx0 = reinterpret_cast<const int32_t *>(lo + S - 4);    // the last word of member 0's slice
        Lookahead a;
        a.slabs_now_hold(NextBatch{stage0, idx0, 6}, true);
        a.announce(s1);
        const Lookahead r = a.rebased(lo, S, 2);
        CHECK(r.slabs_hold(NextBatch{reinterpret_cast<const float *>(lo + 2 * S + 64), reinterpret_cast<const int32_t *>(lo + 3 * S - 4), 6}));
        CHECK(r.next == s1 && r.have_next && r.xstage_valid && r.xstage_cur == 1);
        CHECK(a.rebased(lo, S, 0) == a);
        Lookahead e;                                                             // one byte past the slice is not member 0's
        e.slabs_now_hold(NextBatch{reinterpret_cast<const float *>(lo + S), nullptr, 6}, false);
        CHECK(e.rebased(lo, S, 1) == e);
    }
    { // the same transitions on member 0 and on member k's own rebased pointers: rebased(m0, k) == mk; on one only: not equal
        const char *lo = arena.data();
        const int k = 2;
        auto stage = [&](int m) { return NextBatch{reinterpret_cast<const float *>(lo + (size_t)m * S + 64), nullptr, 6}; };
        Lookahead m0, mk;
        m0.announce(s0); mk.announce(s0);                                        // (the device ring is shared)
        NextBatch n0{}, nk{};
        m0.slabs_now_hold(stage(0), false); mk.slabs_now_hold(stage(k), false);
        CHECK(m0.rebased(lo, S, k) == mk && !(m0 == mk));
        CHECK(m0.take_next(&n0) && mk.take_next(&nk) && n0 == nk);
        m0.slabs_now_hold(n0, true); mk.slabs_now_hold(nk, true);
        m0.announce(s1); mk.announce(s1);
        CHECK(m0.rebased(lo, S, k) == mk && m0 == mk);                           // (only shared pointers left)
        mk.step_takes_slabs();
        CHECK(!(m0.rebased(lo, S, k) == mk));
        m0.step_takes_slabs();
        CHECK(m0.rebased(lo, S, k) == mk);
        m0.take_next(&n0);
        CHECK(!(m0.rebased(lo, S, k) == mk));
        mk.take_next(&nk);
        m0.slabs_now_hold(n0, true);
        CHECK(!(m0.rebased(lo, S, k) == mk));                                    // (the staging buffer index differs too)
        mk.slabs_now_hold(nk, true);
        CHECK(m0.rebased(lo, S, k) == mk);
        mk.step_left_no_slabs();
        CHECK(!(m0.rebased(lo, S, k) == mk));
    }
    if (g_failed) { std::printf("%d checks failed\n", g_failed); return 1; }
    std::printf("lookahead ok\n");
    return 0;
}
