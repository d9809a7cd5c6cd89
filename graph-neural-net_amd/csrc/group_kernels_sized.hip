// group_kernels_sized.hip -- the SIZED grouped instances of the two-launch step (group_kernels.h: every member with its own row
// count, GroupRows) and their launches, for calls with one batch size per member (gnn_mlp_group_train_sampled_sizes): the twins
// of group_kernels.hip's instances, in a unit of their own so that the two compile side by side.  (The prebuilt
// GeneralNeuralNet row-block instances: group_kernels_sized_gnn.hip.)
#include "static_shapes.h"

namespace gnn {
namespace host {

// the sized twin of rb_group_function's choice
const void *rb_group_sized_function(const gnn_mlp *h) {
    if (!h->rb) return nullptr;
    const bool bf = h->dtype == GNN_DTYPE_BF16, softmax = h->out_kind == GNN_OUT_SOFTMAX_CE;
    if (h->rb_static) {
        const int which = static_shape_of(h);
        if (which < 0) return nullptr;
        return softmax ? rb_static_table<RbGroupSized, 0>(which, h->inner_act, bf) : rb_group_sized_static_general(which, h->inner_act, bf);
    }
    return softmax ? rb_runtime_instance<RbGroupSized, 0>(h->L, bf) : rb_runtime_instance<RbGroupSized, 1>(h->L, bf);
}

struct TileGroupSizedF32 {
    static constexpr bool kPeerForms = false;
    template <int S, int D, bool F> static const void *fn() { return GNN_KERNEL(tile_step_group_sized_kernel<S, D, F>); }
};
struct TileGroupSizedBf16 {
    static constexpr bool kPeerForms = false;
    template <int S, int D, bool F> static const void *fn() { return GNN_KERNEL(tile_step_bf16_group_sized_kernel<S, D, F>); }
};

// Member k's row counts as the loop set them (GroupLaunch::rows / next_rows).  own_next: the launch forms the slabs of the batch
// being stepped (the forward-only launch at the start of a chain), not of the announced one.
static GroupRows group_rows(const GroupLaunch &g, bool own_next) {
    GroupRows r{};
    for (int k = 0; k < g.K; k++) { r.rows[k] = g.rows[k]; r.next_rows[k] = own_next ? g.rows[k] : g.next_rows[k]; }
    return r;
}

// one row of workgroups per member, as many as the member with the most rows needs (the others' workgroups past their own
// batch return at once), padded to a multiple of 8 as in launch_rowblock_group
void launch_rowblock_group_sized(gnn_mlp *h, void *const *head_and_params) {
    const GroupLaunch &g = *h->grp;
    GroupRows gr = group_rows(g, false);
    int most = 0;
    for (int k = 0; k < g.K; k++) most = gr.rows[k] > most ? gr.rows[k] : most;
    const unsigned grid = (unsigned)(pad_up(most) / 4);
    GroupArgs ga = group_args(g, (int)grid, 1, gr.rows);
    void *args[12];
    for (int i = 0; i < 10; i++) args[i] = head_and_params[i];
    args[10] = &ga;
    args[11] = &gr;
    const unsigned gx = (grid + 7) / 8 * 8;
    launch_instance(h, -1, g.rb_fn_sized, nullptr, dim3(gx, (unsigned)g.K), dim3(RB_NT), h->rb_lds_bytes, args);
}

void launch_tile_step_group_sized(gnn_mlp *h, int gsrc, int gdst, bool fwd, unsigned grid, const TileStepParams &t) {
    const GroupLaunch &g = *h->grp;
    GroupRows gr = group_rows(g, gsrc == 0);
    const GroupArgs ga = group_args(g, (int)grid, 1, gr.rows);
    const void *fn = h->dtype == GNN_DTYPE_BF16 ? tile_step_instance<TileGroupSizedBf16>(gsrc, gdst, fwd) : tile_step_instance<TileGroupSizedF32>(gsrc, gdst, fwd);
    TileStepParams tp = t;
    void *args[] = {&tp, const_cast<GroupArgs *>(&ga), &gr};
    launch_instance(h, -1, fn, nullptr, dim3(grid, (unsigned)g.K), dim3(TS_THREADS), 0, args);
}

} // namespace host
} // namespace gnn
