// group_eval.hip -- evaluation of a group of nets (include/gnn_mlp.h: gnn_mlp_group_evaluate_range, _ensemble_range): every
// member's accuracy and loss sum and the ensemble's mean output over rows of the group's data set, in one pass.
//
// Two forms, one combine kernel.  Where group_forward_kernel applies (GroupEvalPlan below) a block of rows is TWO launches:
// the grouped forward pass (every member, blockIdx.y = k) into the group's workspace, then group_combine_kernel.  Otherwise
// the members run one after another, each its own do_forward under its EvalScope in blocks of its own eval_block_rows, and
// the same combine kernel reads the members' own prob / lossv / labels buffers: the same results up to near-ties, no speed-up.
// Evaluation writes no weight, no momentum, no step count and no look-ahead state.
// gnn_mlp_group_confusion_range is the same pass with one more launch per block behind the combine kernel: confusion_kernel
// (confusion_kernel.h) over the label tables the combine kernel just read and the ensemble's labels it just wrote.
//
// The validation pass of a group's observed training loop (group.hip: gnn_mlp_group_train_sampled_observed) is enqueued from
// here too: the forward kernel's LOSS_ONLY form into a row of the curve matrix, and group_curve_sum_kernel over that matrix.
#include "handle.h"
#include "confusion_kernel.h"
#include "distill_kernel.h"

#include <algorithm>
#include <memory>

using namespace gnn;
using namespace gnn::host;

namespace {

// Routing (f32 nets): blocks of more rows than this take the member-after-member form even where the kernel applies -- the
// lone per-layer GEMM chain fills the chip at thousands of rows.  Measured crossover (tools/bench_group_eval.py, MI355X, K = 4
// and 16): at 10 000 rows the grouped pass is 1.03-1.40x the K lone calls, at 60 000 rows (blocks of 16 384) 0.75-0.88x; bf16
// groups gain at every size.  The crossover is only bracketed -- it lies between 10 000 and 16 384 rows --
// and the constant sits at the measured lower end: a block of 12 000 rows is routed away without a measurement of its own.
// The two forms agree up to f32 summation order, so for f32 groups the low bits of a row's outputs depend on which side of
// this constant the requested range falls; within one form they depend on nothing but the row.
constexpr int kGroupedMaxBlockRowsF32 = 10000;

// GroupEvalPlan: does group_forward_kernel apply to this net?  Its limits (ge_lds): 3 to 8 layers, at most 16 outputs, data
// rows of at most 1024 padded inputs, hidden layers of at most 1024, and the two activation images + the weight / row chunks
// within 160 KiB of LDS -- with tiles of 32 rows if that fits, else of 16.  Every net of the two-launch training path passes.
struct GroupEvalPlan {
    bool ok = false; int mt = 0; GroupEvalLds lds{}; const void *fn = nullptr, *fn_loss = nullptr;
};
template <bool LOSS_ONLY> const void *forward_instance(bool bf, int mt) {
    return bf ? (mt == 2 ? reinterpret_cast<const void *>(group_forward_kernel<2, true, LOSS_ONLY>) : reinterpret_cast<const void *>(group_forward_kernel<1, true, LOSS_ONLY>))
              : (mt == 2 ? reinterpret_cast<const void *>(group_forward_kernel<2, false, LOSS_ONLY>) : reinterpret_cast<const void *>(group_forward_kernel<1, false, LOSS_ONLY>));
}
GroupEvalPlan make_plan(const gnn_mlp *h) {
    GroupEvalPlan pl;
    const bool bf = h->dtype == GNN_DTYPE_BF16;
    for (int mt = 2; mt >= 1 && !pl.ok; mt--) {
        const GroupEvalLds m = ge_lds(h->ld.data(), h->L, bf, mt);
        if (!m.ok) continue;
        pl.ok = true; pl.mt = mt; pl.lds = m;
        pl.fn = forward_instance<false>(bf, mt);
        pl.fn_loss = forward_instance<true>(bf, mt);
    }
    return pl;
}

int block_cap(const gnn_mlp *h0) { return std::max(h0->max_batch, h0->eval_rows_cap); } // (as eval_block_rows, for both dtypes)

int ensure_workspace(gnn_mlp_group *g, int rows) {
    const int want = pad_up(rows);
    if (g->eval_ws_rows >= want) return GNN_OK;
    HIP_TRY(hipStreamSynchronize(g->stream)); // (a smaller workspace may still be read by a queued pass)
    if (g->eval_ws) (void)hipFree(g->eval_ws);
    g->eval_ws = nullptr; g->eval_ws_rows = 0;
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&g->eval_ws), sizeof(float) * (size_t)g->K * want * 18));
    g->eval_ws_rows = want;
    return GNN_OK;
}

// what both forms of the forward kernel take: the block's rows [first, first + B) of the resident set, the net, the LDS plan
GroupEvalParams forward_params(const gnn_mlp_group *g, const ResidentSet &rs, int64_t first, int B) {
    const gnn_mlp *h0 = g->m[0];
    const int Lm = h0->L - 1;
    const bool bf = h0->dtype == GNN_DTYPE_BF16;
    GroupEvalParams p{};
    p.X = bf ? static_cast<const void *>(rs.Xb + (size_t)first * h0->ld[0]) : static_cast<const void *>(rs.X + (size_t)first * h0->ld[0]);
    p.Y = rs.Y + (size_t)first * h0->ld[Lm]; p.ldy = h0->ld[Lm];
    p.W = bf ? static_cast<const void *>(h0->Wb) : static_cast<const void *>(h0->W);
    p.S = g->S;
    p.rows = B; p.L = h0->L;
    for (int l = 0; l < h0->L; l++) { p.d[l] = h0->dims[l]; p.ld[l] = h0->ld[l]; }
    for (int l = 0; l < Lm; l++) p.w_off[l] = (unsigned)h0->w_off[l];
    p.inner_act = h0->inner_act; p.last_act = h0->last_act; p.out_kind = h0->out_kind;
    const GroupEvalLds &m = g->eval_plan.lds;
    p.off_img[0] = m.off_img[0]; p.off_img[1] = m.off_img[1]; p.ldi[0] = m.ldi[0]; p.ldi[1] = m.ldi[1];
    p.off_w = m.off_w; p.off_x = m.off_x; p.off_z = m.off_z;
    return p;
}

struct EvalOut { // device results of one call
    unsigned long long *hits; double *sums; double *slots; // [K + 1], [K], [n_slots][GE_GROUP_MAX]
    float *mean; int32_t *ens_label;                       // [n][d_out], [n] or null
    unsigned long long *confusion = nullptr;               // [K + 1][d_out][d_out] or null: the members', then the ensemble's (needs ens_label)
    int32_t *member_labels = nullptr;                      // [K][n] or null (with confusion only)
    float *blend_y = nullptr; float keep = 0.f;            // gnn_mlp_group_distill_range: row `first` of the expected rows the mean is blended into (needs mean)
};

// which form a pass over n rows takes, and its block size
struct BlockForm { bool grouped; int block; };
BlockForm block_form(const gnn_mlp_group *g, int64_t n) {
    const gnn_mlp *h0 = g->m[0];
    const int cap = block_cap(h0);
    const bool grouped = g->eval_plan.ok && (h0->dtype == GNN_DTYPE_BF16 || std::min<int64_t>(cap, n) <= kGroupedMaxBlockRowsF32);
    return BlockForm{grouped, grouped ? (int)std::min<int64_t>(cap, n) : eval_block_rows(h0, n)};
}

// rows [first, first + n) of `rs` in blocks: forward (grouped or member after member), then the combine kernel
int run_blocks(gnn_mlp_group *g, const ResidentSet &rs, int64_t first, int64_t n, const EvalOut &o) {
    gnn_mlp *h0 = g->m[0];
    const int Lm = h0->L - 1, ldo = h0->ld[Lm], d_out = h0->dims[Lm];
    const BlockForm form = block_form(g, n);
    const bool grouped = form.grouped;
    const int block = form.block;
    std::vector<std::unique_ptr<EvalScope>> scopes;
    if (grouped) {
        TRY(ensure_workspace(g, block));
    } else {
        for (gnn_mlp *h : g->m) {
            int rc = GNN_OK;
            scopes.emplace_back(new EvalScope(h, block, &rc));
            if (rc != GNN_OK) return rc;
        }
    }
    GroupCombineParams cp{};
    cp.K = g->K; cp.n_out = d_out; cp.ldy = ldo; cp.hits = o.hits; cp.loss_slots = o.slots;
    int slot = 0;
    for (int64_t off = 0; off < n; off += block) {
        const int B = (int)std::min<int64_t>(block, n - off);
        const float *y = rs.Y + (size_t)(first + off) * ldo;
        if (grouped) {
            const size_t cap_rows = (size_t)g->eval_ws_rows;
            GroupEvalParams p = forward_params(g, rs, first + off, B);
            p.out = g->eval_ws; p.loss = g->eval_ws + cap_rows * 16;
            p.label = reinterpret_cast<int32_t *>(g->eval_ws + cap_rows * 17);
            p.ws_stride = cap_rows * 18;
            const GroupEvalLds &m = g->eval_plan.lds;
            const int R = 16 * g->eval_plan.mt;
            void *args[] = {&p};
            HIP_TRY(hipLaunchKernel(g->eval_plan.fn, dim3((unsigned)((B + R - 1) / R), (unsigned)g->K), dim3(GE_NT), args,
                                    (size_t)m.bytes, h0->stream));
            for (int k = 0; k < g->K; k++) {
                cp.out[k] = p.out + (size_t)k * p.ws_stride;
                cp.loss[k] = p.loss + (size_t)k * p.ws_stride;
                cp.label[k] = p.label + (size_t)k * p.ws_stride;
            }
            cp.ld_out = 16;
        } else {
            for (int k = 0; k < g->K; k++) {
                gnn_mlp *h = g->m[(size_t)k];
                do_forward(h, rs.X + (size_t)(first + off) * h->ld[0], y, B, true, true, true);
                TRY_LAUNCHES(h);
                cp.out[k] = h->prob; cp.loss[k] = h->lossv; cp.label[k] = h->labels;
            }
            cp.ld_out = ldo;
        }
        cp.rows = B; cp.Y = y; cp.slot0 = slot;
        cp.mean_out = o.mean ? o.mean + (size_t)off * d_out : nullptr;
        cp.ens_label = o.ens_label ? o.ens_label + off : nullptr;
        const int nb = (B + 255) / 256;
        hipLaunchKernelGGL(group_combine_kernel, dim3((unsigned)nb), dim3(256), 0, h0->stream, cp);
        HIP_TRY(hipGetLastError());
        slot += nb;
        if (o.blend_y) // (distill_kernel.h; the block's expected rows, which the forward and combine launches above have read)
            HIP_TRY(launch_blend(BlendParams{cp.mean_out, o.blend_y + (size_t)off * ldo, ldo, d_out, B, o.keep}, h0->stream));
        if (o.confusion) { // the tables the combine kernel just read, then the ensemble's labels of this block
            ConfusionParams cf{};
            for (int k = 0; k < g->K; k++) cf.label[k] = cp.label[k];
            cf.label[g->K] = cp.ens_label;
            cf.T = g->K + 1; cf.rows = B; cf.n_out = d_out; cf.Y = y; cf.ldy = ldo;
            cf.counts = o.confusion;
            cf.labels_out = o.member_labels; cf.T_copy = g->K; cf.out_stride = n; cf.row_offset = off;
            HIP_TRY(launch_confusion(cf, h0->stream));
        }
    }
    hipLaunchKernelGGL(group_loss_finish_kernel, dim3(1), dim3(64), 0, h0->stream, o.slots, slot, g->K, o.sums);
    HIP_TRY(hipGetLastError());
    return GNN_OK;
}

int n_slots_for(const gnn_mlp_group *g, int64_t n) { // an upper bound over both forms' block sizes
    const int64_t block = std::max<int64_t>(1, std::min<int64_t>(g->m[0]->max_batch, n));
    return (int)((n + block - 1) / block + (n + 255) / 256 + 1);
}

int check_eval_args(gnn_mlp_group *g, int set, int64_t first, int64_t n) {
    if (!g) return fail(GNN_ERR_BAD_ARG, "null group");
    HIP_TRY(hipSetDevice(g->device));
    for (gnn_mlp *h : g->m) TRY(check_handle(h)); // (a member's deferred host-batch update is applied first)
    return check_set_rows(g->m[0], set, first, n);
}

} // namespace

namespace gnn {
namespace host {

void plan_group_eval(gnn_mlp_group *g) {
    const GroupEvalPlan pl = make_plan(g->m[0]);
    g->eval_plan.ok = false;
    if (!pl.ok) return;
    if (hipFuncSetAttribute(pl.fn, hipFuncAttributeMaxDynamicSharedMemorySize, pl.lds.bytes) != hipSuccess ||
        hipFuncSetAttribute(pl.fn_loss, hipFuncAttributeMaxDynamicSharedMemorySize, pl.lds.bytes) != hipSuccess) {
        (void)hipGetLastError();
        return;
    }
    g->eval_plan.ok = true; g->eval_plan.mt = pl.mt; g->eval_plan.lds = pl.lds; g->eval_plan.fn = pl.fn; g->eval_plan.fn_loss = pl.fn_loss;
}

// Always the grouped form, whatever n: a block is the evaluation block of run_blocks, for f32 nets capped where run_blocks
// leaves the grouped form -- a row's loss does not depend on the block it is in.  Never do_forward: member 0 launches for the
// group while the training loop runs (GroupLaunch), and its own forward path would become grouped launches.
int enqueue_group_validation(gnn_mlp_group *g, int n, float *loss_rows, int64_t stride) {
    const gnn_mlp *h0 = g->m[0];
    int block = block_cap(h0);
    if (h0->dtype != GNN_DTYPE_BF16) block = std::min(block, kGroupedMaxBlockRowsF32);
    const int R = 16 * g->eval_plan.mt;
    for (int off = 0; off < n; off += block) {
        const int B = std::min(block, n - off);
        GroupEvalParams p = forward_params(g, resident_set(h0, GNN_SET_TRAIN), off, B);
        p.loss = loss_rows + off; p.loss_stride = (unsigned)stride;
        void *args[] = {&p};
        HIP_TRY(hipLaunchKernel(g->eval_plan.fn_loss, dim3((unsigned)((B + R - 1) / R), (unsigned)g->K), dim3(GE_NT), args,
                                (size_t)g->eval_plan.lds.bytes, h0->stream));
    }
    return GNN_OK;
}

int enqueue_group_curve_sum(gnn_mlp_group *g, const float *rows, int n_rows, int64_t stride, int n, double *d_out) {
    hipLaunchKernelGGL(group_curve_sum_kernel, dim3((unsigned)n_rows, (unsigned)g->K), dim3(256), 0, g->m[0]->stream,
                       CurveSumParams{rows, (unsigned long long)stride, n, d_out});
    HIP_TRY(hipGetLastError());
    return GNN_OK;
}

void free_group_eval(gnn_mlp_group *g) {
    if (g->eval_ws) (void)hipFree(g->eval_ws);
    g->eval_ws = nullptr; g->eval_ws_rows = 0;
    if (g->held_res) (void)hipFree(g->held_res);
    g->held_res = nullptr; g->held_res_bytes = 0;
}

// A point of the held-out curve (group.hip): gnn_mlp_group_evaluate_set_range's launches over rows [0, n) of the held-out set with
// the results left on the device.  prepare_group_point grows what those launches need -- the group's workspace, or every
// member's evaluation workspace -- so that a point between two steps allocates nothing and waits for nothing.
int group_point_slots(const gnn_mlp_group *g, int64_t n) { return n_slots_for(g, n) * GE_GROUP_MAX; }
int prepare_group_point(gnn_mlp_group *g, int64_t n) {
    const BlockForm form = block_form(g, n);
    if (form.grouped) return ensure_workspace(g, form.block);
    for (gnn_mlp *h : g->m) {
        int rc = GNN_OK;
        EvalScope scope(h, form.block, &rc);
        if (rc != GNN_OK) return rc;
    }
    return GNN_OK;
}
// gnn_mlp_group_ensemble_set_range's pass over another handle's rows, the mean kept on the device and blended block by block
int group_distill_rows(gnn_mlp_group *g, const ResidentSet &rs, int64_t first, int64_t n, float *y_rows, float keep) {
    const gnn_mlp *h0 = g->m[0];
    const int K = g->K, ns = n_slots_for(g, n), d_out = h0->dims[h0->L - 1];
    const size_t head = sizeof(unsigned long long) * (size_t)(K + 1) + sizeof(double) * (size_t)K;
    const size_t slots_b = sizeof(double) * (size_t)ns * GE_GROUP_MAX;
    DevScratch res;
    TRY(res.alloc(head + slots_b + sizeof(float) * (size_t)n * d_out));
    hipStream_t st = h0->stream;
    HIP_TRY(hipMemsetAsync(res.p, 0, head, st));
    EvalOut o{};
    o.hits = res.as<unsigned long long>();
    o.sums = reinterpret_cast<double *>(o.hits + (K + 1));
    o.slots = o.sums + K;
    o.mean = reinterpret_cast<float *>(res.as<char>() + head + slots_b);
    o.blend_y = y_rows; o.keep = keep;
    const int rc = run_blocks(g, rs, first, n, o);
    const hipError_t e = hipStreamSynchronize(st); // (also on failure: the scratch is released when this function returns)
    if (rc != GNN_OK) return rc;
    if (e != hipSuccess) return fail(GNN_ERR_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
    return GNN_OK;
}
int enqueue_group_point(gnn_mlp_group *g, int64_t n, unsigned long long *d_hits, double *d_sums, double *d_slots) {
    EvalOut o{};
    o.hits = d_hits; o.sums = d_sums; o.slots = d_slots;
    return run_blocks(g, resident_set(g->m[0], GNN_SET_HELD_OUT), 0, n, o);
}

} // namespace host
} // namespace gnn

extern "C" {

int gnn_mlp_group_eval_launches(const gnn_mlp_group_t *g) { return !g ? -1 : g->eval_plan.ok ? 2 : 0; }

int gnn_mlp_group_evaluate_range(gnn_mlp_group_t *g, int64_t first, int64_t n, int64_t *member_hits, double *member_loss_sum,
                                 int64_t *ensemble_hits) {
    return gnn_mlp_group_evaluate_set_range(g, GNN_SET_TRAIN, first, n, member_hits, member_loss_sum, ensemble_hits);
}
int gnn_mlp_group_ensemble_range(gnn_mlp_group_t *g, int64_t first, int64_t n, double *mean_out, int32_t *labels) {
    return gnn_mlp_group_ensemble_set_range(g, GNN_SET_TRAIN, first, n, mean_out, labels);
}
int gnn_mlp_group_confusion_range(gnn_mlp_group_t *g, int64_t first, int64_t n, int64_t *member_confusion,
                                  int64_t *ensemble_confusion, int32_t *member_labels) {
    return gnn_mlp_group_confusion_set_range(g, GNN_SET_TRAIN, first, n, member_confusion, ensemble_confusion, member_labels);
}

// the three passes on either resident set of the group (MT:159-197: testOnTrainingData / testOnTestData)
int gnn_mlp_group_evaluate_set_range(gnn_mlp_group_t *g, int set, int64_t first, int64_t n, int64_t *member_hits, double *member_loss_sum,
                                     int64_t *ensemble_hits) { return guarded([&]() -> int {
    if (!g) return fail(GNN_ERR_BAD_ARG, "null group");
    if (!member_hits && !member_loss_sum && !ensemble_hits) return fail(GNN_ERR_BAD_ARG, "every output is null");
    TRY(check_eval_args(g, set, first, n));
    const ResidentSet rs = resident_set(g->m[0], set);
    const int K = g->K, ns = n_slots_for(g, n);
    // [K + 1] hit counters, [K] loss sums (one readback), then the loss slots
    const size_t head = sizeof(unsigned long long) * (size_t)(K + 1) + sizeof(double) * (size_t)K;
    DevScratch res;
    TRY(res.alloc(head + sizeof(double) * (size_t)ns * GE_GROUP_MAX));
    hipStream_t st = g->m[0]->stream;
    HIP_TRY(hipMemsetAsync(res.p, 0, head, st));
    EvalOut o{};
    o.hits = res.as<unsigned long long>();
    o.sums = reinterpret_cast<double *>(o.hits + (K + 1));
    o.slots = o.sums + K;
    TRY(run_blocks(g, rs, first, n, o));
    std::vector<unsigned long long> host((size_t)(2 * K + 1));
    static_assert(sizeof(unsigned long long) == sizeof(double), "one buffer for counters and sums");
    HIP_TRY(hipMemcpyAsync(host.data(), res.p, head, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int k = 0; k < K; k++) {
        if (member_hits) member_hits[k] = (int64_t)host[(size_t)k];
        if (member_loss_sum) std::memcpy(&member_loss_sum[k], &host[(size_t)(K + 1 + k)], sizeof(double));
    }
    if (ensemble_hits) *ensemble_hits = (int64_t)host[(size_t)K];
    return GNN_OK;
}); }

int gnn_mlp_group_ensemble_set_range(gnn_mlp_group_t *g, int set, int64_t first, int64_t n, double *mean_out, int32_t *labels) { return guarded([&]() -> int {
    if (!g) return fail(GNN_ERR_BAD_ARG, "null group");
    if (!mean_out && !labels) return fail(GNN_ERR_BAD_ARG, "every output is null");
    TRY(check_eval_args(g, set, first, n));
    const ResidentSet rs = resident_set(g->m[0], set);
    const gnn_mlp *h0 = g->m[0];
    const int K = g->K, ns = n_slots_for(g, n), d_out = h0->dims[h0->L - 1];
    const size_t head = sizeof(unsigned long long) * (size_t)(K + 1) + sizeof(double) * (size_t)K;
    const size_t slots_b = sizeof(double) * (size_t)ns * GE_GROUP_MAX;
    const size_t mean_b = sizeof(float) * (size_t)n * d_out, lab_b = sizeof(int32_t) * (size_t)n;
    DevScratch res;
    TRY(res.alloc(head + slots_b + mean_b + lab_b));
    hipStream_t st = h0->stream;
    HIP_TRY(hipMemsetAsync(res.p, 0, head, st));
    EvalOut o{};
    o.hits = res.as<unsigned long long>();
    o.sums = reinterpret_cast<double *>(o.hits + (K + 1));
    o.slots = o.sums + K;
    o.mean = reinterpret_cast<float *>(res.as<char>() + head + slots_b);
    o.ens_label = reinterpret_cast<int32_t *>(res.as<char>() + head + slots_b + mean_b);
    TRY(run_blocks(g, rs, first, n, o));
    std::vector<char> host(mean_b + lab_b); // (one readback: the mean rows and the labels lie side by side)
    HIP_TRY(hipMemcpyAsync(host.data(), o.mean, mean_b + lab_b, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (mean_out) {
        const float *src = reinterpret_cast<const float *>(host.data());
        for (size_t i = 0; i < (size_t)n * d_out; i++) mean_out[i] = (double)src[i];
    }
    if (labels) std::memcpy(labels, host.data() + mean_b, lab_b);
    return GNN_OK;
}); }

int gnn_mlp_group_confusion_set_range(gnn_mlp_group_t *g, int set, int64_t first, int64_t n, int64_t *member_confusion,
                                      int64_t *ensemble_confusion, int32_t *member_labels) { return guarded([&]() -> int {
    if (!g) return fail(GNN_ERR_BAD_ARG, "null group");
    if (!member_confusion && !ensemble_confusion && !member_labels) return fail(GNN_ERR_BAD_ARG, "every output is null");
    TRY(check_eval_args(g, set, first, n));
    const ResidentSet rs = resident_set(g->m[0], set);
    const gnn_mlp *h0 = g->m[0];
    const int K = g->K, ns = n_slots_for(g, n), d_out = h0->dims[h0->L - 1];
    const size_t cells = (size_t)d_out * d_out;
    // the loss slots | [K + 1] hit counters, [K] loss sums, [K + 1] matrices (one fill) | the members' labels (with the
    // matrices: one readback) | the ensemble's labels
    const size_t slots_b = sizeof(double) * (size_t)ns * GE_GROUP_MAX;
    const size_t head = sizeof(unsigned long long) * (size_t)(K + 1) + sizeof(double) * (size_t)K;
    const size_t conf_b = sizeof(unsigned long long) * (size_t)(K + 1) * cells;
    const size_t lab_b = member_labels ? sizeof(int32_t) * (size_t)K * (size_t)n : 0, ens_b = sizeof(int32_t) * (size_t)n;
    DevScratch res;
    TRY(res.alloc(slots_b + head + conf_b + lab_b + ens_b));
    hipStream_t st = h0->stream;
    HIP_TRY(hipMemsetAsync(res.as<char>() + slots_b, 0, head + conf_b, st));
    EvalOut o{};
    o.slots = res.as<double>();
    o.hits = reinterpret_cast<unsigned long long *>(res.as<char>() + slots_b);
    o.sums = reinterpret_cast<double *>(o.hits + (K + 1));
    o.confusion = reinterpret_cast<unsigned long long *>(res.as<char>() + slots_b + head);
    o.member_labels = member_labels ? reinterpret_cast<int32_t *>(res.as<char>() + slots_b + head + conf_b) : nullptr;
    o.ens_label = reinterpret_cast<int32_t *>(res.as<char>() + slots_b + head + conf_b + lab_b);
    TRY(run_blocks(g, rs, first, n, o));
    std::vector<unsigned long long> host((conf_b + lab_b + 7) / 8);
    HIP_TRY(hipMemcpyAsync(host.data(), o.confusion, conf_b + lab_b, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (member_confusion) for (size_t i = 0; i < (size_t)K * cells; i++) member_confusion[i] = (int64_t)host[i];
    if (ensemble_confusion) for (size_t i = 0; i < cells; i++) ensemble_confusion[i] = (int64_t)host[(size_t)K * cells + i];
    if (member_labels) std::memcpy(member_labels, reinterpret_cast<const char *>(host.data()) + conf_b, lab_b);
    return GNN_OK;
}); }

} // extern "C"
