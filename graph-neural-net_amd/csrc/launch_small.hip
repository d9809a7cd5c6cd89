// launch_small.hip -- host side of the small-net path: the row-block kernels (middle4_kernel.h, rowblock_kernel.h, with their
// run-time instantiation, jit.h) and the tile-owner kernel (tile_step_kernel.h).  Which instance runs: the table of
// instances.h / static_shapes.h, asked here for the single-net families; every launch goes through launch_instance (handle.h).
#include "static_shapes.h"
#include "jit.h"

using namespace gnn;
using namespace gnn::host;

namespace gnn {
namespace host {

// ---- middle4_kernel plan ----------------------------------------------------------------------
// (the prebuilt instances and their tables: static_shapes.h; the GeneralNeuralNet ones live in launch_small_gnn.hip)
template <class SH> bool shape_matches(const gnn_mlp *h) {
    constexpr int n = (int)(sizeof(SH::kDims) / sizeof(int));
    if (h->L != n) return false;
    for (int i = 0; i < n; i++) if (h->dims[i] != SH::kDims[i]) return false;
    return true;
}

// 0 / 1: the net has one of the two prebuilt shapes (either output kind); -1: it does not, or GNN_MLP_STATIC=0
int static_shape_of(const gnn_mlp *h) {
    if (h->env_static_off) return -1;
    if (shape_matches<ShapeMnistA>(h)) return 0;
    if (shape_matches<ShapeMnistB>(h)) return 1;
    return -1;
}

const void *mid4_function(const gnn_mlp *h, int variant) {
    const bool softmax = h->out_kind == GNN_OUT_SOFTMAX_CE;
    const int which = static_shape_of(h);
    if (which >= 0) return softmax ? mid4_static_table<0>(which, h->inner_act, variant) : mid4_static_general(which, h->inner_act, variant);
    return softmax ? mid4_runtime_instance<0>(h->L, variant) : mid4_runtime_instance<1>(h->L, variant);
}

// What both row kernels' parameter structs (Mid4Params, RbParams: kernel ABI, same field names) take from the handle.
// At plan time: the middle weights, activations and deltas.
template <class P> void bind_net(const gnn_mlp *h, P &p) {
    const int Lm = h->L - 1;
    for (int l = 1; l < Lm; l++) { p.W[l] = h->W + h->w_off[l]; p.act[l] = h->act[l]; }
    for (int l = 1; l <= Lm; l++) p.delta[l] = h->delta[l];
    if (h->dtype == GNN_DTYPE_BF16) {
        for (int l = 1; l < Lm; l++) { p.Wb[l] = h->Wb + h->w_off[l]; p.actb[l] = h->actb[l]; }
        for (int l = 1; l <= Lm; l++) p.deltab[l] = h->deltab[l];
    }
    p.last_act = h->last_act;
    p.inner_act = h->inner_act;
}
// Per call: the slabs, the batch's expected rows and what the caller wants back.
template <class P> void bind_call(const gnn_mlp *h, P &p, const float *y, int B, bool want_prob, bool want_loss, bool want_label) {
    p.slabs = h->slabs; p.slab_rows = h->cap_rows;
    p.Y = y; p.ldy = h->ld[h->L - 1];
    p.prob = want_prob ? h->prob : nullptr;
    p.loss = want_loss ? h->lossv : nullptr;
    p.label = want_label ? h->labels : nullptr;
    p.B = B;
    p.row_idx = h->cur_idx;
}

void plan_mid4(gnn_mlp *h) {
    h->mid4 = false;
    if (h->env_path == 2) { h->plan_note = "row-block kernel switched off (GNN_MLP_PATH=nomid4)"; return; } // tests: force the per-layer middle
    Mid4Params &m = h->mid4p;
    m = Mid4Params{};
    const bool bf16 = h->dtype == GNN_DTYPE_BF16;
    m.plan = make_mid4_plan(h->dims.data(), h->L, bf16);
    if (!m.plan.ok) return; // (plan_fused notes that the middle weights do not fit LDS)
    h->mid4_lds_bytes = (size_t)m.plan.lds_floats * sizeof(float);
    bind_net(h, m);
    h->specialization = static_shape_of(h) >= 0 ? 1 : 0;
    for (int bwd = (bf16 ? 2 : 0); bwd < 3; bwd++) {
        h->mid4_fn[bwd] = mid4_function(h, (bf16 && bwd == 2) ? 3 : bwd);
        if (hipFuncSetAttribute(h->mid4_fn[bwd], hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)h->mid4_lds_bytes) != hipSuccess) {
            (void)hipGetLastError();
            return;
        }
    }
    h->mid4 = true;
}

// ---- rowblock_kernel plan -----------------------------------------------------------------------
void plan_rowblock(gnn_mlp *h) {
    h->rb = false;
    h->rb_fn = nullptr; h->rb_jit = nullptr; h->rb_static = 0;
    const bool bf = h->dtype == GNN_DTYPE_BF16;
    if (!h->chain || h->env_rb_off) return;
    if (bf && h->L > 4) return; // (the bf16 form covers nets of three and four layers; deeper ones keep middle4_kernel<.., BF16>)
    RbParams &r = h->rbp;
    r = RbParams{};
    r.plan = make_rb_plan(h->dims.data(), h->L);
    if (!r.plan.ok) return; // (the two-launch step then keeps middle4_kernel as its row-block kernel)
    h->rb_lds_bytes = (size_t)r.plan.lds_floats * sizeof(float);
    bind_net(h, r);
    r.slabs = h->slabs; r.slab_rows = h->cap_rows;
    const bool softmax = h->out_kind == GNN_OUT_SOFTMAX_CE;
    const int which = static_shape_of(h);
    if (which >= 0) {
        h->rb_fn = softmax ? rb_static_table<RbSingle, 0>(which, h->inner_act, bf) : rb_static_general(which, h->inner_act, bf);
        h->rb_static = 1;
    }
    else h->rb_fn = softmax ? rb_runtime_instance<RbSingle, 0>(h->L, bf) : rb_runtime_instance<RbSingle, 1>(h->L, bf);
    if (hipFuncSetAttribute(h->rb_fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->rb_lds_bytes) != hipSuccess) {
        (void)hipGetLastError();
        h->rb_fn = nullptr;
        return;
    }
    h->rb = true;
}

// Run-time instantiation of middle4_kernel for this net's shape (jit.h); silent no-op when the
// net is already specialised, does not take the middle4 path, or hiprtc is unavailable.
void try_specialize(gnn_mlp *h) {
    if (h->grp) return; // (a group call launches the grouped instances: group_kernels.h)
    if (!h->mid4 || h->specialization != 0 || h->jit_tried) return;
    h->jit_tried = true;
    if (h->env_jit_off) return;
    const jit::Specialised *sp = jit::get_middle4(h->device, h->dims.data(), h->L, h->inner_act, h->out_kind, h->chain,
                                                  h->dtype == GNN_DTYPE_BF16, h->mid4_lds_bytes);
    if (!sp) return;
    h->mid4_jit[0] = sp->fn[0];
    h->mid4_jit[1] = sp->fn[1];
    h->mid4_jit[2] = sp->fn[2];
    h->specialization = 2;
    if (h->rb && !h->rb_static) { // the training row-block kernel for this shape, from the same embedded sources
        const jit::Specialised *rs = jit::get_rowblock(h->device, h->dims.data(), h->L, h->inner_act, h->out_kind, h->dtype == GNN_DTYPE_BF16, h->rb_lds_bytes);
        if (rs) h->rb_jit = rs->fn[0];
    }
}

// forward of the middle4 path; backward = also delta_1..delta_{L-1}
// from_slabs: A_1 = f(sum of the K slabs) (tile_step_kernel made them); else fwd_first_kernel writes act[1] first
void fused_forward(gnn_mlp *h, const float *a0, const float *y, int B, bool backward, bool want_prob,
                   bool want_loss, bool want_label, bool from_slabs, int copy_rows) {
    if (!from_slabs) launch_fwd_first(h, a0, B);
    if (from_slabs && h->rb) { // the two-launch step's training kernel (rowblock_kernel.h)
        RbParams r = h->rbp;
        bind_call(h, r, y, B, want_prob, want_loss, want_label);
        if (copy_rows == RB_COPY_CURRENT && h->cur_idx) { // the sampled batch's rows, contiguous, for the tile kernel that follows (RbParams::xcopy)
            r.ldx = h->ld[0]; r.copy_idx = h->cur_idx;
            if (h->dtype == GNN_DTYPE_BF16) { r.Xb = a0_bf16(h, a0); r.xcopyb = h->xstage_b[h->la.xstage_cur]; }
            else { r.X = a0; r.xcopy = h->xstage[h->la.xstage_cur]; }
        } else if (copy_rows == RB_COPY_NEXT && h->la.have_next && h->la.next.idx) { // the announced next batch's rows, to the OTHER buffer
            r.ldx = h->ld[0]; r.copy_idx = h->la.next.idx; // (next_B == B: chain_gradient)
            if (h->dtype == GNN_DTYPE_BF16) { r.Xb = a0_bf16(h, h->la.next.a0); r.xcopyb = h->xstage_b[h->la.xstage_cur ^ 1]; }
            else { r.X = h->la.next.a0; r.xcopy = h->xstage[h->la.xstage_cur ^ 1]; }
        }
        // (the head arguments: rowblock_kernel.h, GNN_RB_HEAD_PARAMS -- in this order)
        const bool bf = h->dtype == GNN_DTYPE_BF16; // (the bf16 kernel takes its bf16 shadows' pointers in the two weight slots)
        const float *hd_W1 = bf ? reinterpret_cast<const float *>(r.Wb[1]) : r.W[1];
        const float *hd_Wl = bf ? reinterpret_cast<const float *>(r.Wb[h->L - 2]) : r.W[h->L - 2];
        void *args[] = {&r.slabs, &hd_W1, &hd_Wl, &r.row_idx, &r.Y, &r.copy_idx, &r.B, &r.slab_rows, &r.ldy, &r};
        const unsigned grid = (unsigned)(pad_up(B) / 4);
        if (h->grp) { launch_rowblock_group(h, B, args); return; } // every member of a group (group_kernels.hip)
        launch_instance(h, GNN_K_MIDDLE, h->rb_fn, h->rb_jit, dim3(grid), dim3(RB_NT), h->rb_lds_bytes, args);
        return;
    }
    Mid4Params m4 = h->mid4p;
    for (int l = 1; l < h->L - 1; l++) m4.act[l] = h->act[l]; // (the evaluation workspace may stand in: plan.hip, EvalScope)
    bind_call(h, m4, y, B, want_prob, want_loss, want_label);
    m4.n_slabs = h->n_slabs;
    void *args[] = {&m4};
    const int bw = from_slabs ? 2 : backward ? 1 : 0;
    // every padded row is processed: rows >= B become zeros
    launch_instance(h, GNN_K_MIDDLE, h->mid4_fn[bw], h->mid4_jit[bw], dim3((unsigned)(pad_up(B) / 4)), dim3(1024), h->mid4_lds_bytes, args);
}

// ---- tile_step_kernel launches ------------------------------------------------------------------
// the single-net families of tile_step_instance (instances.h), peer forms included
// (HEAD = false, GNN_MLP_TILE_HEAD=0: the kernels with their earlier prologue -- arguments from the struct, every tile by lookup, W and V at the top)
template <bool HEAD> struct TileF32 {
    static constexpr bool kPeerForms = true;
    template <int S, int D, bool F> static const void *fn() { return GNN_KERNEL(tile_step_kernel<S, D, F, HEAD, HEAD>); }
    static const void *merged() { static_assert(HEAD, "the merged kinds have the head prologue only"); return GNN_KERNEL(tile_step_kernel<1, 2, true, true, true, true, true>); }
};
template <bool HEAD> struct TileBf16 {
    static constexpr bool kPeerForms = true;
    template <int S, int D, bool F> static const void *fn() { return GNN_KERNEL(tile_step_bf16_kernel<S, D, F, HEAD>); }
};

// gsrc / gdst / fwd as in tile_step_kernel.h; fwd_only_layer0: the grid covers layer 0's tiles only
// staged: the current batch's rows come from the contiguous copy xstage[xstage_cur] instead of (a0, cur_idx)
void launch_tile_step(gnn_mlp *h, int gsrc, int gdst, const NextBatch *next, const float *a0, int B, float step_over_b, float momentum,
                      bool staged, const PeerGradients *peers, bool next_staged) {
    TileStepParams t = h->tsp;
    if (peers) {
        for (int r = 0; r < peers->n; r++) t.Gpeer[r] = peers->G[r];
        t.n_peer = peers->n; t.slice = peers->slice; t.Gself = h->G;
    }
    t.layer[0].A = staged ? h->xstage[h->la.xstage_cur] : a0;
    for (int l = 0; l < t.n_layers; l++) t.layer[l].G = h->G + h->w_off[l];
    t.K = pad_up(B); t.k_true = B;
    t.row_idx = staged ? nullptr : h->cur_idx;
    const int stage_dst = h->la.xstage_cur ^ 1; // a sampled next batch is copied to the OTHER buffer (this launch may be reading the current one)
    if (next && next->idx && !h->rb) { t.stage_out = h->xstage[stage_dst]; t.stage_out_b = h->xstage_b[stage_dst]; } // (with the row-block kernel on the path IT makes the copy)
    t.step_over_b = step_over_b; t.momentum = momentum;
    const bool fwd = next != nullptr;
    if (fwd) { t.An = next->a0; t.ldan = h->ld[0]; t.next_idx = next->idx; t.next_rows = next->B; t.next_K = pad_up(next->B); }
    if (fwd && next_staged) { t.An = h->xstage[stage_dst]; t.next_idx = nullptr; } // (the row-block kernel in front of this launch copied the rows)
    const bool fwd_only = gsrc == 0;
    const dim3 grid(fwd_only ? h->ts_tiles0 : h->ts_tiles), block(TS_THREADS);
    if (fwd_only) t.n_layers = 1;
    t.tile_map = fwd_only ? h->ts_map0 : h->ts_map;
    t.map_in_args = h->ts_map_args ? 1 : 0;
    if (h->ts_map_args) std::memcpy(t.map_words, h->ts_map_words[fwd_only ? 1 : 0], sizeof(t.map_words));
    const int cls = fwd_only ? GNN_K_FWD_GEMM0 : gsrc >= 2 ? GNN_K_UPDATE : GNN_K_GRAD_GEMM0;
    if (h->dtype == GNN_DTYPE_BF16) {
        if (staged) t.Ab[0] = h->xstage_b[h->la.xstage_cur];
        else if (a0) t.Ab[0] = a0_bf16(h, a0);
        if (fwd) t.Anb = next_staged ? h->xstage_b[stage_dst] : a0_bf16(h, next->a0);
    }
    if (h->grp) { launch_tile_step_group(h, gsrc, gdst, fwd, grid.x, t, B); return; } // every member of a group (group_kernels.hip)
    const bool bf = h->dtype == GNN_DTYPE_BF16, head = !h->env_tile_head_off;
    // The training form of a single f32 net on the row-block kernel's path: the merged map and the instance that knows its
    // workgroup kinds, when the plan kept one (plan.hip: at most one workgroup per CU).  Same results, tile for tile.
    if (h->ts_merge && h->rb && !bf && !h->group && head && gsrc == 1 && gdst == 2 && fwd && !t.stage_out) {
        std::memcpy(t.map_words, h->ts_merge_words, sizeof(t.map_words));
        t.map_in_args = 1;
        int hd_Kr = t.K | (t.row_idx ? 1 : 0);
        TileHead hd = h->ts_merge_head;
        void *args[] = {&t.layer[0].A, &t.layer[0].D, &t.layer[0].W, &t.layer[0].V, &t.layer[0].lda, &t.layer[0].ldd, &t.layer[0].M, &hd_Kr, &hd.geo, &hd.kx, &t};
        launch_instance(h, cls, tile_step_merged_instance<TileF32<true>>(), nullptr, dim3((unsigned)h->ts_merge_tiles), block, 0, args);
        return;
    }
    const void *fn = bf ? (head ? tile_step_instance<TileBf16<true>>(gsrc, gdst, fwd) : tile_step_instance<TileBf16<false>>(gsrc, gdst, fwd))
                        : (head ? tile_step_instance<TileF32<true>>(gsrc, gdst, fwd) : tile_step_instance<TileF32<false>>(gsrc, gdst, fwd));
    // (the head arguments: tile_step_kernel.h, GNN_TS_HEAD_PARAMS -- in this order; the bf16 kernel takes layer 0's bf16 A and D in the first two slots)
    const GradLayer &l0 = t.layer[0];
    const float *hd_A = bf ? reinterpret_cast<const float *>(t.Ab[0]) : l0.A, *hd_D = bf ? reinterpret_cast<const float *>(t.Db[0]) : l0.D;
    int hd_Kr = t.K | (t.row_idx ? 1 : 0); // (the padded rows are a multiple of 16)
    TileHead hd = h->ts_head[fwd_only ? 1 : 0];
    void *args[] = {&hd_A, &hd_D, &t.layer[0].W, &t.layer[0].V, &t.layer[0].lda, &t.layer[0].ldd, &t.layer[0].M, &hd_Kr, &hd.geo, &hd.kx, &t};
    launch_instance(h, cls, fn, nullptr, grid, block, 0, args);
}

} // namespace host
} // namespace gnn
