// group_sizes.h -- internal: the batch sizes of a group's members, where member 0's look-ahead state (lookahead.h) stands for all.
// A batch in Lookahead is named by address AND size.  Member 0's control path steps the group, so its state names member 0's
// sizes; in a call with one batch size per member (gnn_mlp_group_train_sampled_sizes) member k's batches at the same addresses
// have other sizes.  GroupSizes is the group's record of them: the size, per member, of the batch `slab` names and of the batch
// `next` names in member 0's state.  It answers the three questions the host asks per iteration and per call:
//   * what a step of such a call hands the grouped launches (SizedStep): every member's live rows now and in the announced
//     iteration, and whether "the announced batch has the current batch's size" holds for EVERY member -- what member 0's control
//     path decides from that (plan.hip: rb_next) it decides once for all;
//   * what member k's state is after a grouped call (member_view): member 0's, rebased, with member k's sizes;
//   * whether member 0's state still describes every member before the next one (describes + member_view compared with what the
//     member holds): like is compared with like, so a group whose members have different sizes keeps its state across calls.
// A mistake here never changes a result (lookahead.h).  Plain C++, no HIP: tests/native/group_sizes_check.cpp runs it on the host.
#pragma once
#include "lookahead.h"

namespace gnn {
namespace host {

constexpr int kGroupSizesMax = 16; // (GROUP_MAX of group_kernels.h; group.hip asserts that they agree)

// one iteration of a call with one batch size per member
struct SizedStep {
    int rows[kGroupSizesMax] = {};      // member k's live rows in the iteration being stepped
    int next_rows[kGroupSizesMax] = {}; // ... and in the announced one (zeros: nothing announced)
    bool announced = false;
    bool next_same_rows = true;         // for every member, the announced batch has the current batch's size
};
inline SizedStep make_sized_step(int K, const int *rows, const int *next_rows) {
    SizedStep s;
    s.announced = next_rows != nullptr;
    for (int k = 0; k < K; k++) {
        s.rows[k] = rows[k];
        s.next_rows[k] = next_rows ? next_rows[k] : 0;
        if (!next_rows || next_rows[k] != rows[k]) s.next_same_rows = false;
    }
    return s;
}

struct GroupSizes {
    int slab_B[kGroupSizesMax] = {}, next_B[kGroupSizesMax] = {};

    // member 0's state names one size for all (every grouped call but the sized one; a state that was forgotten)
    void uniform(int K, const Lookahead &m0) {
        for (int k = 0; k < K; k++) { slab_B[k] = m0.slab.B; next_B[k] = m0.next.B; }
    }
    bool is_uniform(int K) const {
        for (int k = 1; k < K; k++) if (slab_B[k] != slab_B[0] || next_B[k] != next_B[0]) return false;
        return true;
    }
    // A step of a sized call went through member 0's control path (plan.hip, chain_gradient).  With a batch announced, the tile
    // launch made the announced batch's slabs: `slab` and `next` both name it.  Without, `slab` names the batch that was stepped
    // (ensure_slabs wrote it, or it was there) and `next` is untouched.
    void stepped(int K, const SizedStep &s) {
        for (int k = 0; k < K; k++) {
            slab_B[k] = s.announced ? s.next_rows[k] : s.rows[k];
            if (s.announced) next_B[k] = s.next_rows[k];
        }
    }
    // member 0's state is the one this record was made for (member 0 stepped alone since: its sizes are its own again)
    bool describes(const Lookahead &m0) const { return m0.slab.B == slab_B[0] && m0.next.B == next_B[0]; }
    // member 0's state as member k holds it: the pointers by Lookahead::rebased, the sizes member k's
    Lookahead member_view(const Lookahead &m0, const char *lo, size_t S, int k, const char *idx_lo = nullptr, size_t idx_S = 0) const {
        Lookahead r = m0.rebased(lo, S, k, idx_lo, idx_S);
        r.slab.B = slab_B[k]; r.next.B = next_B[k];
        return r;
    }
};

} // namespace host
} // namespace gnn
