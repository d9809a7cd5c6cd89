// group_kernels.hip -- the grouped instances of the two-launch step (group_kernels.h) and their launches: the tile kernels
// in the forms a single-GPU chain uses, the row-block kernel for the prebuilt SoftmaxCrossEntropyNeuralNet shapes and for
// runtime extents.  (The prebuilt GeneralNeuralNet row-block instances: group_kernels_gnn.hip, compiled beside this unit; the
// sized twins of all of them, for calls with one batch size per member: group_kernels_sized.hip, group_kernels_sized_gnn.hip.)
// The choices are the single-net ones (instances.h, static_shapes.h) asked for the grouped families; the launches go through
// launch_instance (handle.h) with no timer class: grouped launches are not timed.
#include "static_shapes.h"

namespace gnn {
namespace host {

// the grouped twin of plan_rowblock's choice (launch_small.hip): the prebuilt shape's instance, else the runtime-shape one
const void *rb_group_function(const gnn_mlp *h) {
    if (!h->rb) return nullptr;
    const bool bf = h->dtype == GNN_DTYPE_BF16, softmax = h->out_kind == GNN_OUT_SOFTMAX_CE;
    if (h->rb_static) {
        const int which = static_shape_of(h);
        if (which < 0) return nullptr;
        return softmax ? rb_static_table<RbGroup, 0>(which, h->inner_act, bf) : rb_group_static_general(which, h->inner_act, bf);
    }
    return softmax ? rb_runtime_instance<RbGroup, 0>(h->L, bf) : rb_runtime_instance<RbGroup, 1>(h->L, bf);
}

// the grouped families of tile_step_instance (instances.h): the forms a single-GPU chain uses, no peer forms
struct TileGroupF32 {
    static constexpr bool kPeerForms = false;
    template <int S, int D, bool F> static const void *fn() { return GNN_KERNEL(tile_step_group_kernel<S, D, F>); }
};
struct TileGroupBf16 {
    static constexpr bool kPeerForms = false;
    template <int S, int D, bool F> static const void *fn() { return GNN_KERNEL(tile_step_bf16_group_kernel<S, D, F>); }
};

// the arguments every grouped launch takes; rows: member k's live rows of the batch being stepped (a sized launch), null: B for all
GroupArgs group_args(const GroupLaunch &g, int nbx, int B, const int *rows) {
    GroupArgs a{};
    a.arena_lo = g.arena_lo;
    a.S = g.S;
    a.nbx = nbx;
    a.idx_lo = g.idx_lo;
    a.idx_S = g.idx_S;
    for (int k = 0; k < g.K; k++) { // (as step_on_rows: the caller's step over THIS batch's size)
        a.step_over_b[k] = (float)(g.step[k] / (double)(rows ? rows[k] : B));
        a.momentum[k] = (float)g.momentum[k];
    }
    return a;
}

// one row of workgroups per member; a member's row is padded to a multiple of 8 workgroups, so that workgroup x of every
// member lands on the XCD of member 0's workgroup x (the dispatcher deals workgroups to XCDs round robin)
void launch_rowblock_group(gnn_mlp *h, int B, void *const *head_and_params) {
    const GroupLaunch &g = *h->grp;
    if (g.sized) { launch_rowblock_group_sized(h, head_and_params); return; } // (every member with its own row count: group_kernels_sized.hip)
    const unsigned grid = (unsigned)(pad_up(B) / 4);
    GroupArgs ga = group_args(g, (int)grid, 1, nullptr);
    void *args[11];
    for (int i = 0; i < 10; i++) args[i] = head_and_params[i];
    args[10] = &ga;
    const unsigned gx = (grid + 7) / 8 * 8;
    launch_instance(h, -1, g.rb_fn, nullptr, dim3(gx, (unsigned)g.K), dim3(RB_NT), h->rb_lds_bytes, args); // (grouped launches are not timed)
}

// the tile map already has a multiple of 8 entries (make_tile_map: slots * 8)
void launch_tile_step_group(gnn_mlp *h, int gsrc, int gdst, bool fwd, unsigned grid, const TileStepParams &t, int B) {
    const GroupLaunch &g = *h->grp;
    if (g.sized) { launch_tile_step_group_sized(h, gsrc, gdst, fwd, grid, t); return; }
    const GroupArgs ga = group_args(g, (int)grid, B, nullptr);
    const void *fn = h->dtype == GNN_DTYPE_BF16 ? tile_step_instance<TileGroupBf16>(gsrc, gdst, fwd) : tile_step_instance<TileGroupF32>(gsrc, gdst, fwd);
    TileStepParams tp = t;
    void *args[] = {&tp, const_cast<GroupArgs *>(&ga)};
    launch_instance(h, -1, fn, nullptr, dim3(grid, (unsigned)g.K), dim3(TS_THREADS), 0, args); // (null: the peer forms are not grouped)
}

} // namespace host
} // namespace gnn
