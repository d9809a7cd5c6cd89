// input_grad.hip -- the gradient of calculateLoss with respect to the INPUT (NN:27, SCE:207-220, GNN:230-242): host side of
// input_grad_kernel.h.  Per block of at most max_batch rows: the handle's own gradient computation without an update
// (do_gradient, untouched: every plan leaves delta_1 -- bf16 nets its rounding deltab[1] -- on the device), one launch of
// input_grad_kernel into the handle's gx buffer, then the consumers (saliency_kernel, a device-to-device copy of the rows, for
// groups input_grad_combine_kernel).  No host work between blocks; the results come back in ONE readback at the end of a call.
// Like gnn_mlp_compute_gradient*, a call leaves the gradient buffer holding its last block's weight gradient; it changes no
// weight, momentum, step count or sampler.
// gnn_mlp_integrated_gradients_set_range: per block the first path point into the staging rows, then per point the gradient
// computation on the staging rows and intgrad_kernel (the running sum, the next point in place, last the attribution into gx),
// then the same consumers and, for the completeness check, two forward passes and intgrad_delta_kernel.
#include "handle.h"
#include "input_grad_kernel.h"

#include <algorithm>
#include <cmath>

using namespace gnn;
using namespace gnn::host;

static_assert(IG_GROUP_MAX == GROUP_MAX, "input_grad_kernel.h and group_kernels.h: one member count");

namespace {

// gx: pad(max_batch) x ld[0] floats, an ordinary allocation (never a slice of a group's arena), made on first use
int ensure_gx(gnn_mlp *h) {
    if (h->gx) return GNN_OK;
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&h->gx), sizeof(float) * (size_t)h->cap_rows * h->ld[0]));
    return GNN_OK;
}

// sal[c][i] += |gx[b][i]| over the block's rows of class c, class_rows[c] += their number (either may be null, not both)
void enqueue_saliency(const gnn_mlp *h, hipStream_t stream, const float *gx, const float *y, int B, double *sal,
                      unsigned long long *class_rows) {
    const int Lm = h->L - 1;
    SaliencyParams s{};
    s.GX = gx; s.ldg = h->ld[0];
    s.d0 = h->dims[0]; s.rows = B; s.n_out = h->dims[Lm];
    s.Y = y; s.ldy = h->ld[Lm];
    s.sal = sal; s.class_rows = class_rows;
    const unsigned gx_blocks = sal ? (unsigned)((h->dims[0] + SAL_NT - 1) / SAL_NT) : 1u;
    hipLaunchKernelGGL(saliency_kernel, dim3(gx_blocks, (unsigned)h->dims[Lm]), dim3(SAL_NT), 0, stream, s);
}

// the block's live rows without their padding, behind the rows of the blocks before it
int enqueue_row_copy(const gnn_mlp *h, hipStream_t stream, const float *gx, int B, float *dst) {
    const size_t w = sizeof(float) * (size_t)h->dims[0];
    HIP_TRY(hipMemcpy2DAsync(dst, w, gx, sizeof(float) * (size_t)h->ld[0], w, (size_t)B, hipMemcpyDeviceToDevice, stream));
    return GNN_OK;
}

int check_rows(const gnn_mlp *h, int64_t first, int64_t n) {
    if (!h->DX) return fail(GNN_ERR_STATE, "no dataset uploaded");
    if (n <= 0 || first < 0 || first + n > h->dataset_n) return fail(GNN_ERR_BAD_ARG, "rows outside the dataset");
    return GNN_OK;
}

void widen(const float *src, double *dst, size_t n) {
    for (size_t i = 0; i < n; i++) dst[i] = (double)src[i];
}

// ---- integrated gradients: intgrad_kernel, intgrad_start_kernel, intgrad_delta_kernel ------------------------------------------
constexpr int INTGRAD_MAX_STEPS = 1024;

int ensure_gsum(gnn_mlp *h) {
    if (h->gsum) return GNN_OK;
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&h->gsum), sizeof(float) * (size_t)h->cap_rows * h->ld[0]));
    return GNN_OK;
}

// act[0] = baseline + alpha * (x0 - baseline) of the block's rows, and on a bf16 handle its shadow (the forward passes read it)
void enqueue_intgrad_point(gnn_mlp *h, const float *x0, int B, float alpha, float baseline) {
    IntGradStartParams p{};
    p.X0 = x0; p.ldx0 = h->ld[0];
    p.out = h->act[0]; p.ldo = h->ld[0];
    p.M = h->ld[0]; p.m_true = h->dims[0]; p.rows = B; p.rows_pad = pad_up(B);
    p.alpha = alpha; p.bl = baseline;
    hipLaunchKernelGGL(intgrad_start_kernel, dim3(grid_for((int64_t)p.rows_pad * (p.M / 4))), dim3(256), 0, h->stream, p);
    if (h->dtype == GNN_DTYPE_BF16) to_bf16(h, h->act[0], h->actb[0], (size_t)pad_up(B) * h->ld[0]);
}

// behind a do_gradient on the staging rows: path point k of m -- the sum, then the next point in place or the attribution in gx
void enqueue_intgrad_step(gnn_mlp *h, const float *x0, int B, int k, int m, float alpha_next, float baseline) {
    const bool bf = h->dtype == GNN_DTYPE_BF16;
    IntGradParams q{};
    InputGradParams &p = q.g;
    p.D = bf ? static_cast<const void *>(h->deltab[1]) : static_cast<const void *>(h->delta[1]);
    p.W = bf ? static_cast<const void *>(h->Wb + h->w_off[0]) : static_cast<const void *>(h->W + h->w_off[0]);
    p.A0 = h->act[0]; p.lda = h->ld[0];
    p.GX = h->gx; p.ldg = h->ld[0];
    p.M = h->ld[0]; p.m_true = h->dims[0];
    p.K = h->ld[1];
    p.rows = B;
    p.act = h->inner_act;
    q.A = h->act[0];
    q.X0 = x0; q.ldx0 = h->ld[0];
    q.S = h->gsum; q.lds = h->ld[0];
    q.k = k; q.m = m;
    q.alpha_next = alpha_next; q.bl = baseline; q.mf = (float)m;
    const dim3 grid((unsigned)((h->ld[0] / 16 + IG_WAVES - 1) / IG_WAVES), (unsigned)(pad_up(B) / 16));
    if (bf) hipLaunchKernelGGL(intgrad_kernel<true>, grid, dim3(IG_WAVES * 64), 0, h->stream, q);
    else hipLaunchKernelGGL(intgrad_kernel<false>, grid, dim3(IG_WAVES * 64), 0, h->stream, q);
    if (bf && k < m - 1) to_bf16(h, h->act[0], h->actb[0], (size_t)pad_up(B) * h->ld[0]);
}

} // namespace

namespace gnn {
namespace host {
// gx = (delta_1 . W_0^T) * f'(a0) of the block do_gradient has just run on -- or, `step`, the rows moved along the sign of that
// gradient into step->out (fgsm_kernel, or with an origin pgd_kernel; gx is then neither needed nor written)
void enqueue_input_grad(gnn_mlp *h, const float *a0, int B, const AdvStep *step) {
    const bool bf = h->dtype == GNN_DTYPE_BF16;
    InputGradParams p{};
    p.D = bf ? static_cast<const void *>(h->deltab[1]) : static_cast<const void *>(h->delta[1]);
    p.W = bf ? static_cast<const void *>(h->Wb + h->w_off[0]) : static_cast<const void *>(h->W + h->w_off[0]);
    p.A0 = a0; p.lda = h->ld[0];
    p.GX = step ? step->out : h->gx; p.ldg = h->ld[0];
    p.M = h->ld[0]; p.m_true = h->dims[0];
    p.K = h->ld[1];
    p.rows = B;
    p.act = h->inner_act;
    const dim3 grid((unsigned)((h->ld[0] / 16 + IG_WAVES - 1) / IG_WAVES), (unsigned)(pad_up(B) / 16));
    if (step) {
        const FgsmParams q{p, step->eps, step->lo, step->hi};
        if (step->origin) {
            const PgdParams s{q, step->alpha, step->origin, h->ld[0], step->idx};
            if (bf) hipLaunchKernelGGL(pgd_kernel<true>, grid, dim3(IG_WAVES * 64), 0, h->stream, s);
            else hipLaunchKernelGGL(pgd_kernel<false>, grid, dim3(IG_WAVES * 64), 0, h->stream, s);
        } else if (bf) hipLaunchKernelGGL(fgsm_kernel<true>, grid, dim3(IG_WAVES * 64), 0, h->stream, q);
        else hipLaunchKernelGGL(fgsm_kernel<false>, grid, dim3(IG_WAVES * 64), 0, h->stream, q);
        return;
    }
    if (bf) hipLaunchKernelGGL(input_grad_kernel<true>, grid, dim3(IG_WAVES * 64), 0, h->stream, p);
    else hipLaunchKernelGGL(input_grad_kernel<false>, grid, dim3(IG_WAVES * 64), 0, h->stream, p);
}
void enqueue_pgd_start(gnn_mlp *h, const AdvStep &step, int B, int64_t row0, int64_t seed, int n) {
    PgdStartParams p{};
    p.X0 = step.origin; p.ldx0 = h->ld[0]; p.idx = step.idx;
    p.out = h->act[0]; p.ldo = h->ld[0];
    p.M = h->ld[0]; p.m_true = h->dims[0]; p.rows = B; p.rows_pad = pad_up(B);
    p.row0 = (uint32_t)row0; p.seed = seed < 0 ? 0u : (uint32_t)seed; p.n = (uint32_t)n;
    p.random = seed < 0 ? 0 : 1;
    p.eps = step.eps; p.lo = step.lo; p.hi = step.hi;
    hipLaunchKernelGGL(pgd_start_kernel, dim3(grid_for((int64_t)p.rows_pad * (p.M / 4))), dim3(256), 0, h->stream, p);
}
void free_input_grad(gnn_mlp *h) {
    if (h->gx) (void)hipFree(h->gx);
    if (h->gsum) (void)hipFree(h->gsum);
    h->gx = h->gsum = nullptr;
}
} // namespace host
} // namespace gnn

extern "C" {

int gnn_mlp_input_gradient(gnn_mlp_t *h, const double *X, const double *Y, int B, double *grad) { return guarded([&]() -> int {
    TRY(check_handle(h));
    if (!X || !Y || !grad) return fail(GNN_ERR_BAD_ARG, "null argument (SCE:209)");
    TRY(check_batch(h, B));
    TRY(ensure_gx(h));
    TRY(stage_batch(h, X, Y, B));
    do_gradient(h, h->act[0], h->ybuf, B, false, 0.f, 0.f, false);
    enqueue_input_grad(h, h->act[0], B);
    TRY_LAUNCHES(h);
    const int d0 = h->dims[0], ld0 = h->ld[0];
    std::vector<float> host((size_t)B * ld0);
    HIP_TRY(hipMemcpyAsync(host.data(), h->gx, sizeof(float) * host.size(), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (int b = 0; b < B; b++) widen(host.data() + (size_t)b * ld0, grad + (size_t)b * d0, (size_t)d0);
    return GNN_OK;
}); }

int gnn_mlp_input_gradient_range(gnn_mlp_t *h, int64_t first, int64_t n, double *grad, double *saliency, int64_t *class_rows) {
return guarded([&]() -> int {
    TRY(check_handle(h));
    if (!grad && !saliency && !class_rows) return fail(GNN_ERR_BAD_ARG, "every output is null");
    TRY(check_rows(h, first, n));
    TRY(ensure_gx(h));
    const int Lm = h->L - 1, d0 = h->dims[0], d_out = h->dims[Lm];
    // [d_out x d0 sums][d_out row counts] (one fill) | the rows' gradients without padding: one readback
    const size_t cells = (size_t)d_out * d0;
    static_assert(sizeof(unsigned long long) == sizeof(double), "one buffer for sums and counters");
    const size_t head = sizeof(double) * (cells + (size_t)d_out), grad_b = grad ? sizeof(float) * (size_t)n * d0 : 0;
    DevScratch res;
    TRY(res.alloc(head + grad_b));
    HIP_TRY(hipMemsetAsync(res.p, 0, head, h->stream));
    double *d_sal = res.as<double>();
    unsigned long long *d_rows = reinterpret_cast<unsigned long long *>(d_sal + cells);
    float *d_grad = reinterpret_cast<float *>(res.as<char>() + head);
    const int block = h->max_batch;
    for (int64_t off = 0; off < n; off += block) {
        const int B = (int)std::min<int64_t>(block, n - off);
        const float *a0 = h->DX + (size_t)(first + off) * h->ld[0];
        const float *y = h->DY + (size_t)(first + off) * h->ld[Lm];
        do_gradient(h, a0, y, B, false, 0.f, 0.f, true);
        enqueue_input_grad(h, a0, B);
        if (saliency || class_rows) enqueue_saliency(h, h->stream, h->gx, y, B, saliency ? d_sal : nullptr, class_rows ? d_rows : nullptr);
        if (grad) TRY(enqueue_row_copy(h, h->stream, h->gx, B, d_grad + (size_t)off * d0));
    }
    TRY_LAUNCHES(h);
    std::vector<double> host((head + grad_b + 7) / 8);
    HIP_TRY(hipMemcpyAsync(host.data(), res.p, head + grad_b, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (saliency) std::memcpy(saliency, host.data(), sizeof(double) * cells);
    if (class_rows) {
        const unsigned long long *c = reinterpret_cast<const unsigned long long *>(host.data() + cells);
        for (int i = 0; i < d_out; i++) class_rows[i] = (int64_t)c[i];
    }
    if (grad) widen(reinterpret_cast<const float *>(reinterpret_cast<const char *>(host.data()) + head), grad, (size_t)n * d0);
    return GNN_OK;
}); }

int gnn_mlp_integrated_gradients_set_range(gnn_mlp_t *h, int set, int64_t first, int64_t n, int steps, double baseline,
                                           double *attributions, double *maps, int64_t *class_rows, double *delta) {
return guarded([&]() -> int {
    TRY(check_handle(h));
    if (!attributions && !maps && !class_rows && !delta) return fail(GNN_ERR_BAD_ARG, "every output is null");
    TRY(check_adv_net(h));
    if (!(baseline >= 0) || !std::isfinite(baseline))
        return fail(GNN_ERR_BAD_ARG, "baseline must be finite and not negative: the device holds f(x), which is x on non-negative values only");
    if (steps < 1 || steps > INTGRAD_MAX_STEPS) return fail(GNN_ERR_BAD_ARG, "steps must lie in 1 .. 1024");
    TRY(check_set_rows(h, set, first, n));
    TRY(ensure_gx(h));
    TRY(ensure_gsum(h));
    const ResidentSet rs = resident_set(h, set);
    const int Lm = h->L - 1, d0 = h->dims[0], d_out = h->dims[Lm], m = steps;
    const float bl = (float)baseline;
    std::vector<float> alpha((size_t)m + 1, 0.f); // alpha_k = (float)((k + 0.5) / m); alpha_m is never used
    for (int k = 0; k < m; k++) alpha[k] = (float)(((double)k + 0.5) / (double)m);
    // [d_out x d0 sums][d_out row counts] (one fill) | n deltas | the rows' attributions without padding: one readback;
    // behind them, not read back, the rows' losses L_x
    const size_t cells = (size_t)d_out * d0;
    static_assert(sizeof(unsigned long long) == sizeof(double), "one buffer for sums and counters");
    const size_t head = sizeof(double) * (cells + (size_t)d_out), delta_b = delta ? sizeof(double) * (size_t)n : 0;
    const size_t attr_b = attributions ? sizeof(float) * (size_t)n * d0 : 0, lx_b = delta ? sizeof(float) * (size_t)n : 0;
    DevScratch res;
    TRY(res.alloc(head + delta_b + attr_b + lx_b));
    HIP_TRY(hipMemsetAsync(res.p, 0, head, h->stream));
    double *d_sal = res.as<double>();
    unsigned long long *d_rows = reinterpret_cast<unsigned long long *>(d_sal + cells);
    double *d_delta = reinterpret_cast<double *>(res.as<char>() + head);
    float *d_attr = reinterpret_cast<float *>(res.as<char>() + head + delta_b);
    float *d_lx = reinterpret_cast<float *>(res.as<char>() + head + delta_b + attr_b);
    const int block = h->max_batch;
    for (int64_t off = 0; off < n; off += block) {
        const int B = (int)std::min<int64_t>(block, n - off);
        const float *x0 = rs.X + (size_t)(first + off) * h->ld[0];
        const float *y = rs.Y + (size_t)(first + off) * h->ld[Lm];
        enqueue_intgrad_point(h, x0, B, alpha[0], bl);
        for (int k = 0; k < m; k++) {
            do_gradient(h, h->act[0], y, B, false, 0.f, 0.f, false);
            enqueue_intgrad_step(h, x0, B, k, m, alpha[(size_t)k + 1], bl);
        }
        if (maps || class_rows) enqueue_saliency(h, h->stream, h->gx, y, B, maps ? d_sal : nullptr, class_rows ? d_rows : nullptr);
        if (attributions) TRY(enqueue_row_copy(h, h->stream, h->gx, B, d_attr + (size_t)off * d0));
        if (delta) { // the completeness check: the losses of the rows and of the baseline rows (gx is no forward pass's buffer)
            do_forward(h, x0, y, B, false, true, false);
            HIP_TRY(hipMemcpyAsync(d_lx + off, h->lossv, sizeof(float) * (size_t)B, hipMemcpyDeviceToDevice, h->stream));
            enqueue_intgrad_point(h, x0, B, 0.f, bl);
            do_forward(h, h->act[0], y, B, false, true, false);
            const IntGradDeltaParams dp{h->gx, h->ld[0], d0, B, d_lx + off, h->lossv, d_delta + off};
            hipLaunchKernelGGL(intgrad_delta_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, h->stream, dp);
        }
    }
    TRY_LAUNCHES(h);
    const size_t back = head + delta_b + attr_b;
    std::vector<double> host((back + 7) / 8);
    HIP_TRY(hipMemcpyAsync(host.data(), res.p, back, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (maps) std::memcpy(maps, host.data(), sizeof(double) * cells);
    if (class_rows) {
        const unsigned long long *c = reinterpret_cast<const unsigned long long *>(host.data() + cells);
        for (int i = 0; i < d_out; i++) class_rows[i] = (int64_t)c[i];
    }
    const char *tail = reinterpret_cast<const char *>(host.data()) + head;
    if (delta) std::memcpy(delta, tail, delta_b);
    if (attributions) widen(reinterpret_cast<const float *>(tail + delta_b), attributions, (size_t)n * d0);
    return GNN_OK;
}); }

int gnn_mlp_group_input_gradient_range(gnn_mlp_group_t *g, int64_t first, int64_t n, double *member_grad, double *ensemble_grad,
                                       double *member_saliency, double *ensemble_saliency, int64_t *class_rows) {
return guarded([&]() -> int {
    if (!g) return fail(GNN_ERR_BAD_ARG, "null group");
    if (!member_grad && !ensemble_grad && !member_saliency && !ensemble_saliency && !class_rows)
        return fail(GNN_ERR_BAD_ARG, "every output is null");
    HIP_TRY(hipSetDevice(g->device));
    for (gnn_mlp *h : g->m) TRY(check_handle(h)); // (a member's deferred host-batch update is applied first)
    gnn_mlp *h0 = g->m[0];
    TRY(check_rows(h0, first, n));
    const int K = g->K, Lm = h0->L - 1, d0 = h0->dims[0], d_out = h0->dims[Lm], ld0 = h0->ld[0];
    int block = h0->max_batch;
    for (gnn_mlp *h : g->m) { TRY(ensure_gx(h)); block = std::min(block, h->max_batch); }
    hipStream_t st = h0->stream;
    // [K + 1 maps of d_out x d0 sums][d_out row counts] (one fill) | the members' rows | the ensemble's rows: one readback
    const size_t cells = (size_t)d_out * d0, rows_f = (size_t)n * d0;
    const size_t head = sizeof(double) * ((size_t)(K + 1) * cells + (size_t)d_out);
    const size_t mg_b = member_grad ? sizeof(float) * (size_t)K * rows_f : 0, eg_b = ensemble_grad ? sizeof(float) * rows_f : 0;
    const bool want_ens = ensemble_grad || ensemble_saliency;
    DevScratch res, ens;
    TRY(res.alloc(head + mg_b + eg_b));
    if (want_ens) TRY(ens.alloc(sizeof(float) * (size_t)pad_up(block) * ld0));
    HIP_TRY(hipMemsetAsync(res.p, 0, head, st));
    double *d_sal = res.as<double>();
    unsigned long long *d_rows = reinterpret_cast<unsigned long long *>(d_sal + (size_t)(K + 1) * cells);
    float *d_mg = reinterpret_cast<float *>(res.as<char>() + head);
    float *d_eg = reinterpret_cast<float *>(res.as<char>() + head + mg_b);
    for (int64_t off = 0; off < n; off += block) {
        const int B = (int)std::min<int64_t>(block, n - off);
        const float *y = h0->DY + (size_t)(first + off) * h0->ld[Lm];
        unsigned long long *count_here = class_rows ? d_rows : nullptr; // the block's rows are counted by ONE of its launches
        InputGradCombineParams cp{};
        for (int k = 0; k < K; k++) { // the members one after the other, each through its own handle on the group's stream
            gnn_mlp *h = g->m[k];
            const float *a0 = h->DX + (size_t)(first + off) * ld0;
            do_gradient(h, a0, h->DY + (size_t)(first + off) * h->ld[Lm], B, false, 0.f, 0.f, true);
            enqueue_input_grad(h, a0, B);
            if (member_saliency) { enqueue_saliency(h, h->stream, h->gx, y, B, d_sal + (size_t)k * cells, count_here); count_here = nullptr; }
            if (member_grad) TRY(enqueue_row_copy(h, h->stream, h->gx, B, d_mg + (size_t)k * rows_f + (size_t)off * d0));
            cp.gx[k] = h->gx;
        }
        if (want_ens) {
            cp.K = K; cp.ens = ens.as<float>(); cp.n4 = (long long)pad_up(B) * ld0 / 4;
            hipLaunchKernelGGL(input_grad_combine_kernel, dim3((unsigned)((cp.n4 + 255) / 256)), dim3(256), 0, st, cp);
            if (ensemble_saliency) { enqueue_saliency(h0, st, cp.ens, y, B, d_sal + (size_t)K * cells, count_here); count_here = nullptr; }
            if (ensemble_grad) TRY(enqueue_row_copy(h0, st, cp.ens, B, d_eg + (size_t)off * d0));
        }
        if (count_here) enqueue_saliency(h0, st, h0->gx, y, B, nullptr, count_here);
    }
    for (gnn_mlp *h : g->m) TRY_LAUNCHES(h);
    std::vector<double> host((head + mg_b + eg_b + 7) / 8);
    HIP_TRY(hipMemcpyAsync(host.data(), res.p, head + mg_b + eg_b, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (member_saliency) std::memcpy(member_saliency, host.data(), sizeof(double) * (size_t)K * cells);
    if (ensemble_saliency) std::memcpy(ensemble_saliency, host.data() + (size_t)K * cells, sizeof(double) * cells);
    if (class_rows) {
        const unsigned long long *c = reinterpret_cast<const unsigned long long *>(host.data() + (size_t)(K + 1) * cells);
        for (int i = 0; i < d_out; i++) class_rows[i] = (int64_t)c[i];
    }
    const char *rows = reinterpret_cast<const char *>(host.data()) + head;
    if (member_grad) widen(reinterpret_cast<const float *>(rows), member_grad, (size_t)K * rows_f);
    if (ensemble_grad) widen(reinterpret_cast<const float *>(rows + mg_b), ensemble_grad, rows_f);
    return GNN_OK;
}); }

} // extern "C"
