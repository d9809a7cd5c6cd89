// lookahead.h -- internal: what the host knows about the work the two-launch step has done ahead.  The tile kernel of step s also
// forms the first-layer K slabs of step s + 1's batch; whether a step may use them, and which batch the next tile launch prepares,
// is decided from this state alone.  The member functions are the ONLY code that writes it, each named for its cause.  A mistake
// here never changes a result: it costs a forward-only launch (tests/test_launch_counts_gpu.py counts them).  Plain C++, no HIP.
#pragma once
#include <cstddef>
#include <cstdint>

namespace gnn {
namespace host {
struct NextBatch { const float *a0; const int32_t *idx; int B; }; // a batch by address: rows of A_0, optionally through a device index vector
inline bool operator==(const NextBatch &x, const NextBatch &y) { return x.a0 == y.a0 && x.idx == y.idx && x.B == y.B; }

struct Lookahead {
    bool slab_valid = false; NextBatch slab{}; // the batch whose first-layer sums (for the CURRENT weights) the slabs hold
    bool have_next = false; NextBatch next{};  // the batch the next gradient computation will run on (gnn_mlp_hint_next_range, train loops)
    // gnn_mlp::xstage[xstage_cur] holds the rows of the (sampled) batch the slabs describe; the other buffer takes the next copy
    int xstage_cur = 0; bool xstage_valid = false;

    bool slabs_hold(const NextBatch &b) const { return slab_valid && slab == b; }
    void announce(const NextBatch &b) { have_next = true; next = b; }
    // the launch that updates the weights takes the announcement: it is good for ONE weight update
    bool take_next(NextBatch *b) { if (!have_next) return false; have_next = false; *b = next; return true; }
    // a launch made the slabs of `b` from the current weights; staged_copy: it (or the row-block kernel in front of it) also wrote
    // the batch's rows to the OTHER staging buffer, which becomes the current one
    void slabs_now_hold(const NextBatch &b, bool staged_copy) { slab_valid = true; slab = b; xstage_cur ^= (int)staged_copy; xstage_valid = staged_copy; }
    // One gradient computation on the two-launch path (plan.hip, chain_gradient).  Its row kernel is about to read the slabs, and
    // the weights they were made from are about to change:
    void step_takes_slabs() { slab_valid = false; }
    // ... it ended without slabs for a next batch (none announced; a gradient of rows in a staging buffer): the staged rows are stale
    void step_left_no_slabs() { xstage_valid = false; }
    // ... it left the weights unchanged on resident rows: the slabs (and, `staged`, the staged rows) still describe `b`
    void step_kept_weights(const NextBatch &b, bool staged) { slab_valid = true; slab = b; xstage_valid = staged; }
    // the batch comes from the host, or the net is off the two-launch path: a hint names dataset rows for a chain step
    void hint_unused() { have_next = false; }
    // slabs of rows in a host staging buffer, used by this very call: the buffer holds other rows under the same address at the next
    void slabs_of_staging_buffer() { slab_valid = false; xstage_valid = false; }
    void weights_replaced() { slab_valid = false; } // W set from outside: first-layer sums made with the old weights
    // addresses no longer name the rows they named (dataset upload, idxbuf reused, the device index ring released), or a kernel that
    // prepares nothing updated the weights (flat / direct update): neither slabs nor hint describe anything
    void rows_renamed() { slab_valid = false; have_next = false; }
    // gnn_mlp_forget_lookahead; a deferred update applied on its own: results unchanged, the next step opens a chain
    void forget() { slab_valid = false; have_next = false; xstage_valid = false; }

    // Groups (group.hip): member k's buffers lie at member 0's + k * S, member 0's inside the arena slice [lo, lo + S); what every
    // member shares (the dataset, the device index ring) lies outside and keeps its address.  Member 0's state as member k holds it:
    // A call with one sampler per member (gnn_mlp_group_train_sampled_each) has a second such range while it runs: the device
    // index region, member 0's ring in [idx_lo, idx_lo + idx_S), member k's at + k * idx_S.  Only the index pointers follow it;
    // idx_S == 0: no region, the rule above alone.  (Invalidated entries are moved too: operator== compares them.)
    Lookahead rebased(const char *lo, size_t S, int k, const char *idx_lo = nullptr, size_t idx_S = 0) const {
        auto moved = [&](auto *p) {
            const bool own = p && (size_t)(reinterpret_cast<const char *>(p) - lo) < S;
            return own ? reinterpret_cast<decltype(p)>(reinterpret_cast<const char *>(p) + (size_t)k * S) : p;
        };
        auto moved_idx = [&](const int32_t *p) {
            const bool ring = p && (size_t)(reinterpret_cast<uintptr_t>(p) - reinterpret_cast<uintptr_t>(idx_lo)) < idx_S;
            return ring ? reinterpret_cast<const int32_t *>(reinterpret_cast<const char *>(p) + (size_t)k * idx_S) : moved(p);
        };
        Lookahead r = *this;
        r.slab.a0 = moved(slab.a0); r.slab.idx = moved_idx(slab.idx); r.next.a0 = moved(next.a0); r.next.idx = moved_idx(next.idx);
        return r;
    }
    // the device index region of such a call is released: as rows_renamed, and no entry keeps an address inside it (a later
    // comparison between members, enter_grouped, knows of no region any more)
    void index_region_released() { rows_renamed(); slab.idx = nullptr; next.idx = nullptr; }
    bool operator==(const Lookahead &o) const {
        return slab_valid == o.slab_valid && have_next == o.have_next && xstage_valid == o.xstage_valid && slab == o.slab && next == o.next && xstage_cur == o.xstage_cur;
    }
};
} // namespace host
} // namespace gnn
