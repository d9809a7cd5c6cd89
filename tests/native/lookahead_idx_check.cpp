// Host check of the index-range form of Lookahead::rebased (csrc/lookahead.h; tests/test_lookahead_idx_cpu.py compiles and runs
// it): in a group call with one sampler per member, member 0's device index ring is slice 0 of a region of K slices of idx_S
// bytes, and member k's copy of an index pointer into slice 0 lies k * idx_S further on -- while arena pointers go on moving by
// k * S and data-set pointers and null stay.  Stale (invalidated) entries are moved too: operator== compares them.
#include "../../graph-neural-net_amd/csrc/lookahead.h"

#include <cstdio>
#include <vector>

using gnn::host::Lookahead;
using gnn::host::NextBatch;

static int g_failed = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); g_failed++; } \
    } while (0)

int main() {
    std::vector<float> dataset(64);
    const size_t S = 256, IS = 128;                   // bytes per member: arena slice, index slice
    const int K = 3;
    std::vector<char> arena(K * S);
    std::vector<int32_t> region(K * IS / 4);          // K index rings of 32 words
    const char *lo = arena.data(), *ilo = reinterpret_cast<const char *>(region.data());
    const float *dx = dataset.data();
    auto ring = [&](int m, int word) { return region.data() + (size_t)m * (IS / 4) + word; };
    auto own = [&](int m, size_t byte) { return reinterpret_cast<const float *>(lo + (size_t)m * S + byte); };
    auto own_idx = [&](int m, size_t byte) { return reinterpret_cast<const int32_t *>(lo + (size_t)m * S + byte); };

    for (int k = 0; k < K; k++) { // pointers in slice 0 move by k * idx_S, the first and the last word included
        Lookahead a;
        a.slabs_now_hold(NextBatch{dx, ring(0, 0), 6}, true);
        a.announce(NextBatch{dx, ring(0, 31), 5});
        const Lookahead r = a.rebased(lo, S, k, ilo, IS);
        CHECK(r.slabs_hold(NextBatch{dx, ring(k, 0), 6}));
        CHECK(r.have_next && r.next == (NextBatch{dx, ring(k, 31), 5}));
        CHECK(r.xstage_valid && r.xstage_cur == 1);
        CHECK((k == 0) == (r == a));
        CHECK(a.rebased(lo, S, k) == a);              // (without a region the ring is shared: it keeps its address)
    }
    { // one word past slice 0 is not member 0's ring: it stays
        Lookahead a;
        a.slabs_now_hold(NextBatch{dx, ring(1, 0), 6}, false);
        CHECK(a.rebased(lo, S, 2, ilo, IS) == a);
    }
    { // arena pointers move by k * S -- a member's own index buffer too --, data-set pointers and null stay
        Lookahead a;
        a.slabs_now_hold(NextBatch{own(0, 64), own_idx(0, S - 4), 6}, true);
        a.announce(NextBatch{dx + 16, nullptr, 6});
        const Lookahead r = a.rebased(lo, S, 2, ilo, IS);
        CHECK(r.slabs_hold(NextBatch{own(2, 64), own_idx(2, S - 4), 6}));
        CHECK(r.next == (NextBatch{dx + 16, nullptr, 6}));
        CHECK(r == a.rebased(lo, S, 2));              // (nothing of it lies in the region)
    }
    { // k = 0 is the identity, whatever the state holds
        Lookahead a;
        a.slabs_now_hold(NextBatch{own(0, 64), ring(0, 3), 6}, true);
        a.announce(NextBatch{dx, ring(0, 9), 4});
        CHECK(a.rebased(lo, S, 0, ilo, IS) == a);
        CHECK(Lookahead().rebased(lo, S, 0, ilo, IS) == Lookahead());
        CHECK(Lookahead().rebased(lo, S, 2, ilo, IS) == Lookahead());
    }
    { // the same transitions on member 0 (ring 0) and on member k (ring k): rebased(m0, k) == mk after each, stale entries included
        const int k = 2;
        Lookahead m0, mk;
        auto same = [&] { return m0.rebased(lo, S, k, ilo, IS) == mk; };
        m0.slabs_now_hold(NextBatch{dx, ring(0, 0), 6}, true); mk.slabs_now_hold(NextBatch{dx, ring(k, 0), 6}, true);
        CHECK(same() && !(m0 == mk) && !(m0.rebased(lo, S, k) == mk));
        m0.announce(NextBatch{dx, ring(0, 8), 6}); mk.announce(NextBatch{dx, ring(k, 8), 6});
        CHECK(same());
        m0.step_takes_slabs(); mk.step_takes_slabs();  // slab.idx is stale now, and still compared
        CHECK(same() && !(m0.rebased(lo, S, k) == mk));
        NextBatch n0{}, nk{};
        CHECK(m0.take_next(&n0) && mk.take_next(&nk) && n0.idx == ring(0, 8) && nk.idx == ring(k, 8));
        CHECK(same());                                 // next.idx stale on both
        m0.slabs_now_hold(n0, true); mk.slabs_now_hold(nk, true);
        CHECK(same());
        m0.forget(); mk.forget();
        CHECK(same() && !(m0 == mk));                  // (forgetting keeps the addresses: they differ between the members)
        m0.rows_renamed();
        CHECK(same());                                 // (nothing it clears was set)
        mk.slabs_now_hold(NextBatch{dx, ring(k, 16), 6}, false);
        CHECK(!same());
        m0.slabs_now_hold(NextBatch{dx, ring(0, 16), 6}, false);
        CHECK(same());
        // the region is released: no entry keeps an address inside it, and the members agree without a region
        m0.index_region_released(); mk.index_region_released();
        CHECK(m0 == mk && m0.rebased(lo, S, k) == mk && !m0.slab_valid && !m0.have_next);
        CHECK(m0.slab.idx == nullptr && m0.next.idx == nullptr);
    }
    if (g_failed) { std::printf("%d checks failed\n", g_failed); return 1; }
    std::printf("lookahead idx ok\n");
    return 0;
}
