// group_kernels.hip -- the grouped instances of the two-launch step (group_kernels.h) and their launches: the tile kernels
// in the forms a single-GPU chain uses, the row-block kernel for the prebuilt SoftmaxCrossEntropyNeuralNet shapes and for
// runtime extents.  (The prebuilt GeneralNeuralNet row-block instances: group_kernels_gnn.hip, compiled beside this unit.)
#include "static_shapes.h"

namespace gnn {
namespace host {

template <class SH, int OUTK, bool BF> const void *rb_group_fn_static(int act) {
    switch (act) {
    case 0: return reinterpret_cast<const void *>(&rowblock_group_kernel<SH, 0, OUTK, BF>);
    case 1: return reinterpret_cast<const void *>(&rowblock_group_kernel<SH, 1, OUTK, BF>);
    case 2: return reinterpret_cast<const void *>(&rowblock_group_kernel<SH, 2, OUTK, BF>);
    case 3: return reinterpret_cast<const void *>(&rowblock_group_kernel<SH, 3, OUTK, BF>);
    default: return reinterpret_cast<const void *>(&rowblock_group_kernel<SH, 4, OUTK, BF>);
    }
}
template <int NL, bool BF> const void *rb_group_fn_runtime(int out_kind) {
    return out_kind == GNN_OUT_SOFTMAX_CE ? reinterpret_cast<const void *>(&rowblock_group_kernel<RbRuntimeShape<NL>, -1, 0, BF>)
                                          : reinterpret_cast<const void *>(&rowblock_group_kernel<RbRuntimeShape<NL>, -1, 1, BF>);
}

// the grouped twin of plan_rowblock's choice (launch_small.hip): the prebuilt shape's instance, else the runtime-shape one
const void *rb_group_function(const gnn_mlp *h) {
    if (!h->rb) return nullptr;
    const bool bf = h->dtype == GNN_DTYPE_BF16;
    if (h->rb_static) {
        const int which = static_shape_of(h);
        if (which < 0) return nullptr;
        if (h->out_kind != GNN_OUT_SOFTMAX_CE) return rb_group_static_general(which, h->inner_act, bf);
        if (which == 0) return bf ? rb_group_fn_static<RbMnistA, 0, true>(h->inner_act) : rb_group_fn_static<RbMnistA, 0, false>(h->inner_act);
        return bf ? rb_group_fn_static<RbMnistB, 0, true>(h->inner_act) : rb_group_fn_static<RbMnistB, 0, false>(h->inner_act);
    }
    if (bf) return h->L == 3 ? rb_group_fn_runtime<3, true>(h->out_kind) : h->L == 4 ? rb_group_fn_runtime<4, true>(h->out_kind) : nullptr;
    switch (h->L) {
    case 3: return rb_group_fn_runtime<3, false>(h->out_kind);
    case 4: return rb_group_fn_runtime<4, false>(h->out_kind);
    case 5: return rb_group_fn_runtime<5, false>(h->out_kind);
    case 6: return rb_group_fn_runtime<6, false>(h->out_kind);
    default: return rb_group_fn_runtime<0, false>(h->out_kind);
    }
}

static GroupArgs group_args(const GroupLaunch &g, int nbx, int B) {
    GroupArgs a{};
    a.arena_lo = g.arena_lo;
    a.S = g.S;
    a.nbx = nbx;
    for (int k = 0; k < g.K; k++) { // (as step_on_rows: the caller's step over THIS batch's size)
        a.step_over_b[k] = (float)(g.step[k] / (double)B);
        a.momentum[k] = (float)g.momentum[k];
    }
    return a;
}

static void note_launch(gnn_mlp *h, hipError_t le) {
    if (le != hipSuccess && h->launch_error == hipSuccess) h->launch_error = le;
}

// one row of workgroups per member; a member's row is padded to a multiple of 8 workgroups, so that workgroup x of every
// member lands on the XCD of member 0's workgroup x (the dispatcher deals workgroups to XCDs round robin)
void launch_rowblock_group(gnn_mlp *h, unsigned grid, void *const *head_and_params) {
    const GroupLaunch &g = *h->grp;
    GroupArgs ga = group_args(g, (int)grid, 1);
    void *args[11];
    for (int i = 0; i < 10; i++) args[i] = head_and_params[i];
    args[10] = &ga;
    const unsigned gx = (grid + 7) / 8 * 8;
    note_launch(h, hipLaunchKernel(g.rb_fn, dim3(gx, (unsigned)g.K), dim3(RB_NT), args, h->rb_lds_bytes, h->stream));
}

// the tile map already has a multiple of 8 entries (make_tile_map: slots * 8)
void launch_tile_step_group(gnn_mlp *h, int gsrc, int gdst, bool fwd, unsigned grid, const TileStepParams &t, int B) {
    const GroupLaunch &g = *h->grp;
    const GroupArgs ga = group_args(g, (int)grid, B);
    const dim3 gr(grid, (unsigned)g.K), block(TS_THREADS);
    const bool bf = h->dtype == GNN_DTYPE_BF16;
#define GNN_TSG(S, D, F)                                                                                      \
    (bf ? reinterpret_cast<const void *>(&tile_step_bf16_group_kernel<S, D, F>)                              \
        : reinterpret_cast<const void *>(&tile_step_group_kernel<S, D, F>))
    const void *fn = gsrc == 0 ? GNN_TSG(0, 0, true)
                   : gsrc == 1 && gdst == 1 ? GNN_TSG(1, 1, false)
                   : gsrc == 1 && !fwd ? GNN_TSG(1, 2, false)
                   : gsrc == 1 ? GNN_TSG(1, 2, true)
                   : gsrc == 2 && !fwd ? GNN_TSG(2, 2, false)
                   : gsrc == 2 ? GNN_TSG(2, 2, true) : nullptr;
#undef GNN_TSG
    if (!fn) { note_launch(h, hipErrorInvalidValue); return; } // (the peer forms are not grouped)
    TileStepParams tp = t;
    void *args[] = {&tp, const_cast<GroupArgs *>(&ga)};
    note_launch(h, hipLaunchKernel(fn, gr, block, args, 0, h->stream));
}

} // namespace host
} // namespace gnn
