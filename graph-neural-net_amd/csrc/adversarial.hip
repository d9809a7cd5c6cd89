// adversarial.hip -- the fast-gradient-sign perturbation of resident rows on the device: x' = clip(x + eps * sign(g), lo, hi),
// g = d calculateLoss(x, y) / d x (NN:27, SCE:207-220, GNN:230-242; input_grad.hip).  Host side of fgsm_kernel
// (input_grad_kernel.h).  Per block of at most max_batch rows: the handle's own gradient computation without an update
// (do_gradient, untouched), then ONE launch over delta_1 . W_0^T whose epilogue stores the perturbed rows into act[0] instead of
// g; what follows reads act[0] like any host batch (the forward pass of an evaluation, a training step).  No host work between
// blocks or iterations.
// The device holds a0 = f(x), not x (the reference applies f to the raw input too, SCE:183-186): the perturbation is applied
// to a0, which IS x when f is the identity on [0, inf) -- leaky ReLU (MT:235), ReLU, identity -- and the rows and clip bounds
// are non-negative.  Other inner activations are refused; non-negative rows are the caller's precondition.
#include "handle.h"

#include <algorithm>
#include <cmath>

using namespace gnn;
using namespace gnn::host;

namespace gnn {
namespace host {
int check_adv_net(const gnn_mlp *h) {
    if (h->group || h->dp_replica) return fail(GNN_ERR_STATE, "the adversarial calls serve lone nets, not members of a group or replicas");
    if (h->inner_act != GNN_ACT_LEAKY_RELU && h->inner_act != GNN_ACT_RELU && h->inner_act != GNN_ACT_IDENTITY)
        return fail(GNN_ERR_UNSUPPORTED, "the device holds f(x), not x: the perturbation needs an inner activation that is the identity on "
                                         "non-negative inputs (leaky ReLU, ReLU, identity)");
    return GNN_OK;
}
} // namespace host
} // namespace gnn

namespace {

int check_fgsm_args(const gnn_mlp *h, double eps, double lo, double hi, AdvStep *out) {
    TRY(check_adv_net(h));
    if (!(eps >= 0) || !std::isfinite(eps)) return fail(GNN_ERR_BAD_ARG, "eps must be finite and not negative");
    if (!(lo >= 0) || !(hi >= lo)) return fail(GNN_ERR_BAD_ARG, "clip bounds must satisfy 0 <= lo <= hi: the device holds f(x), which is x on non-negative values only");
    *out = AdvStep{(float)eps, (float)lo, (float)hi, h->act[0]};
    return GNN_OK;
}

// act[0] = the perturbation of the block's rows against the current weights; leaves the gradient buffer with the block's weight
// gradient, and the look-ahead state as a gradient computation without an update on the same rows leaves it (`resident`: rows of
// the TRAINING set, the only one the state may name)
void enqueue_fgsm_block(gnn_mlp *h, const float *a0, const float *y, int B, const AdvStep &f, bool resident) {
    do_gradient(h, a0, y, B, false, 0.f, 0.f, resident);
    enqueue_input_grad(h, a0, B, &f);
    if (h->dtype == GNN_DTYPE_BF16) to_bf16(h, h->act[0], h->actb[0], (size_t)pad_up(B) * h->ld[0]); // (the forward passes read the shadow)
}

// One iteration of gnn_mlp_train_sampled_fgsm: the drawn rows gathered into act[0] / ybuf, perturbed in place, stepped on
struct FgsmSampledStep : SampledStep {
    gnn_mlp *h; AdvStep f; double step_size, momentum;
    int step(const int32_t *d_idx, int B) override {
        launch_gather(h, d_idx, B);
        if (h->dtype == GNN_DTYPE_BF16) to_bf16(h, h->act[0], h->actb[0], (size_t)pad_up(B) * h->ld[0]);
        enqueue_fgsm_block(h, h->act[0], h->ybuf, B, f, false);
        return step_on_rows(h, h->act[0], h->ybuf, B, step_size, momentum, false);
    }
};

// ---- the projected attack (PGD; BIM without the random start): pgd_kernel, pgd_start_kernel ------------------------------------
constexpr int PGD_MAX_STEPS = 1024;
struct PgdPlan { AdvStep s; int steps; int64_t seed; };

int check_pgd_args(const gnn_mlp *h, double eps, double alpha, int steps, int64_t start_seed, double lo, double hi, PgdPlan *out) {
    TRY(check_fgsm_args(h, eps, lo, hi, &out->s));
    if (!(alpha >= 0) || !std::isfinite(alpha)) return fail(GNN_ERR_BAD_ARG, "alpha must be finite and not negative");
    if (steps < 0 || steps > PGD_MAX_STEPS) return fail(GNN_ERR_BAD_ARG, "steps must lie in 0 .. 1024");
    if (start_seed >= (int64_t)1 << 31) return fail(GNN_ERR_BAD_ARG, "start_seed must be negative (no random start) or below 2^31");
    out->s.alpha = (float)alpha;
    out->steps = steps;
    out->seed = start_seed < 0 ? -1 : start_seed;
    return GNN_OK;
}

void shadow_rows(gnn_mlp *h, int B) { // (the forward passes of a bf16 handle read the shadow)
    if (h->dtype == GNN_DTYPE_BF16) to_bf16(h, h->act[0], h->actb[0], (size_t)pad_up(B) * h->ld[0]);
}

// act[0] = a_T of the block whose origin rows are `x0` (rows 0 .. B-1, or through `idx`), everything enqueued only.  The start:
// pgd_start_kernel when there is a seed -- or nothing to step from it (steps == 0) or `entry0`, the curve's first entry: the
// origin clipped to the box.  Without a seed the first step reads the iterate from the rows themselves, x0 (resident: rows of the
// training set) or, `gathered`, their copy in act[0]; every later step reads the staging rows.  after(t) follows state t when
// act[0] holds it.
template <class After>
void enqueue_pgd_block(gnn_mlp *h, const PgdPlan &pl, const float *x0, const int32_t *idx, const float *y, int B, int64_t row0, int n,
                       bool resident, bool gathered, bool entry0, After after) {
    AdvStep s = pl.s;
    s.origin = x0; s.idx = idx;
    const float *a = gathered ? h->act[0] : x0;
    bool a_resident = !gathered && resident;
    if (pl.seed >= 0 || pl.steps == 0 || entry0) {
        enqueue_pgd_start(h, s, B, row0, pl.seed, n);
        shadow_rows(h, B);
        if (pl.seed >= 0) { a = h->act[0]; a_resident = false; }
        after(0);
    } else if (gathered) {
        shadow_rows(h, B);
    }
    for (int t = 1; t <= pl.steps; t++) {
        do_gradient(h, a, y, B, false, 0.f, 0.f, a_resident);
        enqueue_input_grad(h, a, B, &s);
        shadow_rows(h, B);
        a = h->act[0]; a_resident = false;
        after(t);
    }
}

// One iteration of gnn_mlp_train_sampled_pgd: the drawn rows gathered, attacked in the staging rows with their origin read from
// the resident rows through the iteration's index vector, stepped on
struct PgdSampledStep : SampledStep {
    gnn_mlp *h; PgdPlan pl; double step_size, momentum; int iteration = 0;
    int step(const int32_t *d_idx, int B) override {
        launch_gather(h, d_idx, B);
        enqueue_pgd_block(h, pl, h->DX, d_idx, h->ybuf, B, 0, iteration++, false, true, false, [](int) {});
        return step_on_rows(h, h->act[0], h->ybuf, B, step_size, momentum, false);
    }
};

} // namespace

extern "C" {

int gnn_mlp_fgsm_set_range(gnn_mlp_t *h, int set, int64_t first, int64_t n, double eps, double lo, double hi, double *X_adv) {
return guarded([&]() -> int {
    TRY(check_handle(h));
    if (!X_adv) return fail(GNN_ERR_BAD_ARG, "null output");
    AdvStep f{};
    TRY(check_fgsm_args(h, eps, lo, hi, &f));
    TRY(check_set_rows(h, set, first, n));
    const ResidentSet rs = resident_set(h, set);
    const int Lm = h->L - 1, d0 = h->dims[0], ld0 = h->ld[0];
    const size_t w = sizeof(float) * (size_t)d0;
    DevScratch res; // the perturbed rows without their padding: one readback
    TRY(res.alloc(w * (size_t)n));
    const int block = h->max_batch;
    for (int64_t off = 0; off < n; off += block) {
        const int B = (int)std::min<int64_t>(block, n - off);
        enqueue_fgsm_block(h, rs.X + (size_t)(first + off) * ld0, rs.Y + (size_t)(first + off) * h->ld[Lm], B, f, set == GNN_SET_TRAIN);
        HIP_TRY(hipMemcpy2DAsync(res.as<float>() + (size_t)off * d0, w, h->act[0], sizeof(float) * (size_t)ld0, w, (size_t)B,
                                 hipMemcpyDeviceToDevice, h->stream));
    }
    TRY_LAUNCHES(h);
    std::vector<float> host((size_t)n * d0);
    HIP_TRY(hipMemcpyAsync(host.data(), res.p, w * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < host.size(); i++) X_adv[i] = (double)host[i];
    return GNN_OK;
}); }

int gnn_mlp_evaluate_fgsm_set_range(gnn_mlp_t *h, int set, int64_t first, int64_t n, double eps, double lo, double hi, int64_t *hits,
                                    double *loss_sum) { return guarded([&]() -> int {
    TRY(check_handle(h));
    if (!hits && !loss_sum) return fail(GNN_ERR_BAD_ARG, "every output is null");
    AdvStep f{};
    TRY(check_fgsm_args(h, eps, lo, hi, &f));
    TRY(check_set_rows(h, set, first, n));
    const ResidentSet rs = resident_set(h, set);
    const int Lm = h->L - 1, d_out = h->dims[Lm];
    DevScratch res; // [hit counter][loss sum]: one fill, one readback
    static_assert(sizeof(unsigned long long) == sizeof(double), "one buffer for the counter and the sum");
    TRY(res.alloc(2 * sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(res.p, 0, 2 * sizeof(unsigned long long), h->stream));
    unsigned long long *d_hits = res.as<unsigned long long>();
    double *d_loss = reinterpret_cast<double *>(d_hits + 1);
    const int block = h->max_batch; // (the gradient computation's buffers hold max_batch rows: no evaluation workspace here)
    for (int64_t off = 0; off < n; off += block) {
        const int B = (int)std::min<int64_t>(block, n - off);
        const float *y = rs.Y + (size_t)(first + off) * h->ld[Lm];
        enqueue_fgsm_block(h, rs.X + (size_t)(first + off) * h->ld[0], y, B, f, set == GNN_SET_TRAIN);
        // the reductions of gnn_mlp_evaluate_set_range (abi.hip: enqueue_evaluation) on the perturbed rows
        do_forward(h, h->act[0], y, B, false, true, true);
        hipLaunchKernelGGL(count_hits_kernel, dim3((B + 255) / 256), dim3(256), 0, h->stream, HitsParams{h->labels, y, h->ld[Lm], d_out, B, d_hits});
        hipLaunchKernelGGL(sum_loss_kernel, dim3(1), dim3(256), 0, h->stream, LossSumParams{h->lossv, B, d_loss, off > 0 ? 1 : 0});
    }
    TRY_LAUNCHES(h);
    unsigned long long host[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(host, res.p, sizeof(host), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (hits) *hits = (int64_t)host[0];
    if (loss_sum) std::memcpy(loss_sum, &host[1], sizeof(double));
    return GNN_OK;
}); }

int gnn_mlp_train_sampled_fgsm(gnn_mlp_t *h, gnn_sampler_t *s, int iterations, int batch, double step, double momentum, double eps,
                               double lo, double hi) { return guarded([&]() -> int {
    TRY(check_handle(h));
    FgsmSampledStep st;
    st.h = h; st.step_size = step; st.momentum = momentum;
    TRY(check_fgsm_args(h, eps, lo, hi, &st.f));
    return train_sampled_run(h, &s, 1, iterations, &batch, step, momentum, 0, nullptr, nullptr, &st);
}); }

int gnn_mlp_pgd_set_range(gnn_mlp_t *h, int set, int64_t first, int64_t n, double eps, double alpha, int steps, int64_t start_seed,
                          double lo, double hi, double *X_adv) { return guarded([&]() -> int {
    TRY(check_handle(h));
    if (!X_adv) return fail(GNN_ERR_BAD_ARG, "null output");
    PgdPlan pl{};
    TRY(check_pgd_args(h, eps, alpha, steps, start_seed, lo, hi, &pl));
    TRY(check_set_rows(h, set, first, n));
    const ResidentSet rs = resident_set(h, set);
    const int Lm = h->L - 1, d0 = h->dims[0], ld0 = h->ld[0];
    const size_t w = sizeof(float) * (size_t)d0;
    DevScratch res; // the attacked rows without their padding: one readback
    TRY(res.alloc(w * (size_t)n));
    const int block = h->max_batch;
    for (int64_t off = 0; off < n; off += block) {
        const int B = (int)std::min<int64_t>(block, n - off);
        enqueue_pgd_block(h, pl, rs.X + (size_t)(first + off) * ld0, nullptr, rs.Y + (size_t)(first + off) * h->ld[Lm], B, first + off, 0,
                          set == GNN_SET_TRAIN, false, false, [](int) {});
        HIP_TRY(hipMemcpy2DAsync(res.as<float>() + (size_t)off * d0, w, h->act[0], sizeof(float) * (size_t)ld0, w, (size_t)B,
                                 hipMemcpyDeviceToDevice, h->stream));
    }
    TRY_LAUNCHES(h);
    std::vector<float> host((size_t)n * d0);
    HIP_TRY(hipMemcpyAsync(host.data(), res.p, w * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < host.size(); i++) X_adv[i] = (double)host[i];
    return GNN_OK;
}); }

int gnn_mlp_evaluate_pgd_set_range(gnn_mlp_t *h, int set, int64_t first, int64_t n, double eps, double alpha, int steps,
                                   int64_t start_seed, double lo, double hi, int curve, int64_t *hits, double *loss_sum) {
return guarded([&]() -> int {
    TRY(check_handle(h));
    if (!hits && !loss_sum) return fail(GNN_ERR_BAD_ARG, "every output is null");
    if (curve != 0 && curve != 1) return fail(GNN_ERR_BAD_ARG, "curve is 0 or 1");
    PgdPlan pl{};
    TRY(check_pgd_args(h, eps, alpha, steps, start_seed, lo, hi, &pl));
    TRY(check_set_rows(h, set, first, n));
    const ResidentSet rs = resident_set(h, set);
    const int Lm = h->L - 1, d_out = h->dims[Lm], T = pl.steps;
    const size_t slots = curve ? (size_t)T + 1 : 1; // entry t: the state after t steps; without a curve the one after step T
    DevScratch res; // [slots hit counters][slots loss sums]: one fill, one readback
    static_assert(sizeof(unsigned long long) == sizeof(double), "one buffer for the counters and the sums");
    TRY(res.alloc(2 * slots * sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(res.p, 0, 2 * slots * sizeof(unsigned long long), h->stream));
    unsigned long long *d_hits = res.as<unsigned long long>();
    double *d_loss = reinterpret_cast<double *>(d_hits + slots);
    const int block = h->max_batch;
    for (int64_t off = 0; off < n; off += block) {
        const int B = (int)std::min<int64_t>(block, n - off);
        const float *y = rs.Y + (size_t)(first + off) * h->ld[Lm];
        enqueue_pgd_block(h, pl, rs.X + (size_t)(first + off) * h->ld[0], nullptr, y, B, first + off, 0, set == GNN_SET_TRAIN, false,
                          curve != 0, [&](int t) {
            if (!curve && t != T) return;
            const size_t slot = curve ? (size_t)t : 0;
            // the reductions of gnn_mlp_evaluate_set_range (abi.hip: enqueue_evaluation) on the state's rows
            do_forward(h, h->act[0], y, B, false, true, true);
            hipLaunchKernelGGL(count_hits_kernel, dim3((B + 255) / 256), dim3(256), 0, h->stream,
                               HitsParams{h->labels, y, h->ld[Lm], d_out, B, d_hits + slot});
            hipLaunchKernelGGL(sum_loss_kernel, dim3(1), dim3(256), 0, h->stream, LossSumParams{h->lossv, B, d_loss + slot, off > 0 ? 1 : 0});
        });
    }
    TRY_LAUNCHES(h);
    std::vector<unsigned long long> host(2 * slots, 0ull);
    HIP_TRY(hipMemcpyAsync(host.data(), res.p, sizeof(unsigned long long) * host.size(), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (hits) for (size_t t = 0; t < slots; t++) hits[t] = (int64_t)host[t];
    if (loss_sum) std::memcpy(loss_sum, host.data() + slots, sizeof(double) * slots);
    return GNN_OK;
}); }

int gnn_mlp_train_sampled_pgd(gnn_mlp_t *h, gnn_sampler_t *s, int iterations, int batch, double step, double momentum, double eps,
                              double alpha, int steps, int64_t start_seed, double lo, double hi) { return guarded([&]() -> int {
    TRY(check_handle(h));
    PgdSampledStep st;
    st.h = h; st.step_size = step; st.momentum = momentum;
    TRY(check_pgd_args(h, eps, alpha, steps, start_seed, lo, hi, &st.pl));
    return train_sampled_run(h, &s, 1, iterations, &batch, step, momentum, 0, nullptr, nullptr, &st);
}); }

} // extern "C"
