// input_grad_kernel.h -- which inputs the loss depends on: g = d calculateLoss(x, y) / d x (NN:27, SCE:207-220, GNN:230-242),
// the l = 0 continuation of the backward loop the reference stops at delta_1 (SCE:272-278), and what consumes it on the device
// (input_grad.hip: gnn_mlp_input_gradient*, gnn_mlp_group_input_gradient_range, gnn_mlp_integrated_gradients_set_range;
// adversarial.hip: gnn_mlp_fgsm_set_range ...).
//   input_grad_kernel<BF>      gx[b][i] = f'(a0[b][i]) * sum_j delta_1[b][j] * W_0[i][j]: pad(B) rows, ld[0] columns, contraction
//                              over ld[1].  f' from a0 = f(x) (the reference applies f to the raw input too, SCE:183-186): for the
//                              leaky pair `a <= 0 ? 0.01 : 1` (MT:235), so an exact-zero pixel gets 0.01.  Both operands are
//                              k-contiguous in memory -- a row of delta_1, a row of W_0 -- and go from global memory straight to
//                              registers in MFMA fragment form, 16 B per lane (8 B of bf16), lane group q taking k = 4q..4q+3 of a
//                              16-deep chunk for BOTH operands (fused_kernels.h: any assignment of k to slots is valid when the
//                              operands agree).  No LDS, no barrier.  W_0 is the ROW operand (as in the tile kernel): a lane's four
//                              accumulators are four consecutive columns of one output row, so a0 is one 16-B load and gx one
//                              16-B store.  One wave per 16 x 16 output tile, the four waves of a workgroup on four neighbouring
//                              column tiles of the same 16 rows.  BF: the operands are the bf16 shadows (deltab[1], Wb), widened
//                              to f32 on the way into v_mfma_f32_16x16x4_f32 -- a product of two bf16 values is exact in f32, the
//                              accumulation is f32 either way, and one kernel body serves both; f' from the unrounded a0.
//                              Rows >= `rows` and columns >= m_true are written as exact zeros (W_0's pad rows are 0).
//   fgsm_kernel<BF>            the same product (ig_tile_product) with the perturbation a0 + eps * sign(g), clipped, as its epilogue
//   pgd_kernel<BF>             ... with one step of the projected attack as its epilogue: a + alpha * sign(g), projected onto the
//                              eps-ball around the row's ORIGIN (read from the resident rows, through the index vector for a
//                              sampled batch), then clipped
//   pgd_start_kernel           element-wise: the attack's start rows, the origin plus eps * u from a counter-based hash, clipped
//   intgrad_kernel<BF>         ... with one path point of integrated gradients as its epilogue: the running sum of g, the next
//                              point into the staging rows, on the last point the attribution (x0 - baseline) * mean g
//   intgrad_start_kernel       element-wise: a path point baseline + alpha * (x0 - baseline) (the first one; alpha 0: the baseline)
//   intgrad_delta_kernel       thread per row: sum of the row's attributions in fp64 minus (loss(x) - loss(baseline))
//   saliency_kernel            thread (column i, class c) walks the block's rows in row order and adds (double)|gx[b][i]| of the
//                              rows whose expected class (confusion_kernel.h: expected_class, MT:186-188) is c into sal[c][i];
//                              the running sum starts from the value the previous block left, so over a range it is ONE sum in row
//                              order per cell: no atomics, the same bits every time.  (A thread per cell, not per column: a
//                              column's d_out sums are independent, and a cell's sum needs one register instead of a map row in
//                              memory.)  Thread 0 of the first column block also counts the class's rows.
//   input_grad_combine_kernel  the ensemble's gradient from a table of the members' gx: s = g_0; s += g_k in member order;
//                              s / (float)K -- the rule of the ensemble's mean output (group_eval_kernel.h).
#pragma once
#include "confusion_kernel.h"

namespace gnn {

constexpr int IG_WAVES = 4;  // waves (column tiles) per workgroup
constexpr int IG_MAXC = 8;   // 16-deep chunks whose loads are in flight at once (IG_MAXC * (4 + 4) VGPRs)
constexpr int IG_GROUP_MAX = 16; // (= GROUP_MAX of group_kernels.h)

struct InputGradParams {
    const void *D;   // delta_1 rows, k-contiguous, leading dimension K: float, or __bf16 (BF)
    const void *W;   // W_0 rows, k-contiguous, leading dimension K: float, or __bf16 (BF)
    const float *A0; int lda; // a0 = f(x) of the block's rows (read for rows < `rows` only)
    float *GX; int ldg;       // pad(rows) x M
    int M, m_true;   // ld[0], d_0
    int K;           // ld[1]: a multiple of 16
    int rows;        // live rows of the block
    int act;
};

template <bool BF> __device__ __forceinline__ f32x4 ig_load4(const void *base, size_t elem) {
    if constexpr (BF) {
        typedef __bf16 ig_bf16x4 __attribute__((ext_vector_type(4)));
        const ig_bf16x4 v = *reinterpret_cast<const ig_bf16x4 *>(static_cast<const __bf16 *>(base) + elem);
        return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
    } else {
        return *reinterpret_cast<const f32x4 *>(static_cast<const float *>(base) + elem);
    }
}

// One wave's 16 x 16 tile of delta_1 . W_0^T at (input columns i0.., batch rows b0..): the loads and the accumulation order every
// kernel over this product shares (input_grad_kernel, fgsm_kernel), so that their g agree bit for bit
template <bool BF> __device__ __forceinline__ f32x4 ig_tile_product(const InputGradParams &p, int i0, int b0, int fr, int fq) {
    const size_t w_at = (size_t)(i0 + fr) * p.K + 4 * fq, d_at = (size_t)(b0 + fr) * p.K + 4 * fq;
    const int nc = p.K / 16;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    for (int cb = 0; cb < nc; cb += IG_MAXC) {
        f32x4 w[IG_MAXC], d[IG_MAXC];
#pragma unroll
        for (int i = 0; i < IG_MAXC; i++) {
            if (cb + i < nc) {
                w[i] = ig_load4<BF>(p.W, w_at + (size_t)(cb + i) * 16);
                d[i] = ig_load4<BF>(p.D, d_at + (size_t)(cb + i) * 16);
            } else {
                w[i] = f32x4{0.f, 0.f, 0.f, 0.f};
                d[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
#pragma unroll
        for (int i = 0; i < IG_MAXC; i++) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (i & 1) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w[i][j], d[i][j], acc1, 0, 0, 0);
                else acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w[i][j], d[i][j], acc0, 0, 0, 0);
            }
        }
    }
    return acc0 + acc1;
}

// grid: (ceil(M / 16 / IG_WAVES), pad(rows) / 16)
template <bool BF>
static __global__ __launch_bounds__(IG_WAVES * 64) void input_grad_kernel(InputGradParams p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int i0 = (blockIdx.x * IG_WAVES + wave) * 16, b0 = blockIdx.y * 16;
    if (i0 >= p.M) return; // (no barrier below)
    const f32x4 acc = ig_tile_product<BF>(p, i0, b0, fr, fq);
    // C / D layout: column (here: batch row) = lane & 15, rows (here: input columns) = 4 * (lane >> 4) + r
    const int b = b0 + fr, col = i0 + 4 * fq;
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (b < p.rows) {
        const f32x4 a = *reinterpret_cast<const f32x4 *>(p.A0 + (size_t)b * p.lda + col);
#pragma unroll
        for (int r = 0; r < 4; r++) o[r] = col + r < p.m_true ? acc[r] * act_prime_from_a(p.act, a[r]) : 0.f;
    }
    *reinterpret_cast<f32x4 *>(p.GX + (size_t)b * p.ldg + col) = o;
}

// The fast-gradient-sign perturbation (adversarial.hip) as the epilogue of the same product: g is formed exactly as above and
// never stored; what is stored, into a ROWS buffer (g.GX, leading dimension g.ldg -- the handle's act[0]), is
//   a' = min(max(a0 + eps * s(g), lo), hi),   s(g) = (g > 0) - (g < 0)
// in f32, every operation rounded on its own.  s(0) = 0 and a NaN g leave the element unperturbed (clipped only).
struct FgsmParams {
    InputGradParams g; // GX / ldg: the perturbed rows
    float eps, lo, hi;
};
__device__ inline float fgsm_value(float a, float g, float eps, float lo, float hi) {
#pragma clang fp contract(off) // (a + eps * s must not become an fma: the formula rounds the product)
    const float s = g > 0.f ? 1.f : g < 0.f ? -1.f : 0.f;
    const float t = eps * s;
    const float v = a + t;
    return fminf(fmaxf(v, lo), hi);
}
// grid as input_grad_kernel's.  In place (g.GX == g.A0, the host-batch case) is safe: a lane reads its own four a0 values, and
// nothing else of A0, before it stores the same four cells; rows >= `rows` and columns >= m_true become exact zeros.
template <bool BF>
static __global__ __launch_bounds__(IG_WAVES * 64) void fgsm_kernel(FgsmParams q) {
    const InputGradParams &p = q.g;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int i0 = (blockIdx.x * IG_WAVES + wave) * 16, b0 = blockIdx.y * 16;
    if (i0 >= p.M) return; // (no barrier below)
    const f32x4 acc = ig_tile_product<BF>(p, i0, b0, fr, fq);
    const int b = b0 + fr, col = i0 + 4 * fq;
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (b < p.rows) {
        const f32x4 a = *reinterpret_cast<const f32x4 *>(p.A0 + (size_t)b * p.lda + col);
#pragma unroll
        for (int r = 0; r < 4; r++)
            o[r] = col + r < p.m_true ? fgsm_value(a[r], acc[r] * act_prime_from_a(p.act, a[r]), q.eps, q.lo, q.hi) : 0.f;
    }
    *reinterpret_cast<f32x4 *>(p.GX + (size_t)b * p.ldg + col) = o;
}

// One step of the projected attack (adversarial.hip: gnn_mlp_pgd_set_range ...) as the epilogue of the same product.  `a` is the
// current iterate (f.g.A0), x0 the ORIGIN of the row -- row `idx ? idx[b] : b` of X0, the resident rows: the staging rows no
// longer hold it after the first step -- and g the gradient at `a`, formed exactly as above.  In f32, every operation rounded on
// its own:
//   v  = a + alpha * s(g)
//   w  = min(max(v, x0 - eps), x0 + eps)     the ball around the origin, each bound one rounding
//   a' = min(max(w, lo), hi)                 the box last: alpha == eps on a == x0 is fgsm_value bit for bit (v is one of the bounds or x0)
struct PgdParams {
    FgsmParams f;    // f.g.A0: the iterate; f.g.GX / ldg: the next iterate
    float alpha;
    const float *X0; int ldx0; // the origin rows (leading dimension ldx0 >= f.g.M)
    const int32_t *idx;        // the block's rows of X0, or null: rows 0 .. rows-1
};
__device__ inline float pgd_value(float a, float x0, float g, float alpha, float eps, float lo, float hi) {
#pragma clang fp contract(off)
    const float s = g > 0.f ? 1.f : g < 0.f ? -1.f : 0.f;
    const float t = alpha * s;
    const float v = a + t;
    const float below = x0 - eps, above = x0 + eps;
    const float w = fminf(fmaxf(v, below), above);
    return fminf(fmaxf(w, lo), hi);
}
// grid as input_grad_kernel's.  In place (f.g.GX == f.g.A0, every step but the first of a range call without a random start) is
// safe for fgsm_kernel's reason: a lane reads its own four cells of A0 and of the origin before it stores the same four cells, and
// X0 is never the buffer written.  idx[b] is loaded for b < rows only; rows >= `rows` and columns >= m_true become exact zeros.
template <bool BF>
static __global__ __launch_bounds__(IG_WAVES * 64) void pgd_kernel(PgdParams q) {
    const InputGradParams &p = q.f.g;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int i0 = (blockIdx.x * IG_WAVES + wave) * 16, b0 = blockIdx.y * 16;
    if (i0 >= p.M) return; // (no barrier below)
    const f32x4 acc = ig_tile_product<BF>(p, i0, b0, fr, fq);
    const int b = b0 + fr, col = i0 + 4 * fq;
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (b < p.rows) {
        const size_t origin = q.idx ? (size_t)q.idx[b] : (size_t)b;
        const f32x4 a = *reinterpret_cast<const f32x4 *>(p.A0 + (size_t)b * p.lda + col);
        const f32x4 x0 = *reinterpret_cast<const f32x4 *>(q.X0 + origin * q.ldx0 + col);
#pragma unroll
        for (int r = 0; r < 4; r++)
            o[r] = col + r < p.m_true ? pgd_value(a[r], x0[r], acc[r] * act_prime_from_a(p.act, a[r]), q.alpha, q.f.eps, q.f.lo, q.f.hi) : 0.f;
    }
    *reinterpret_cast<f32x4 *>(p.GX + (size_t)b * p.ldg + col) = o;
}

// The start of the attack, element-wise, 16 B per lane over the pad(rows) x M staging rows: a_0 = min(max(x0 + eps * u, lo), hi)
// with u in [-1, 1) from a counter-based hash of (seed, n, R, c) -- R the row's index in its resident set (row0 + b, or idx[b]),
// c the column, n the iteration's number (0 for the range calls) -- in uint32 arithmetic that wraps:
//   mix(u):  u ^= u >> 16; u *= 0x7feb352d; u ^= u >> 15; u *= 0x846ca68b; u ^= u >> 16
//   r = mix(mix(mix(seed) + n) ^ R);  h = mix(r + 0x9E3779B9 * c);  u = float(h >> 8) * 2^-23 - 1      (exact)
// `random` == 0: a_0 = x0 clipped to the box alone (steps == 0 without a seed).  Padding rows and columns: exact zeros.
struct PgdStartParams {
    const float *X0; int ldx0; const int32_t *idx; // the origin rows, as in PgdParams
    float *out; int ldo;                           // pad(rows) x M
    int M, m_true, rows, rows_pad;
    uint32_t row0, seed, n;
    int random;
    float eps, lo, hi;
};
__device__ __host__ inline uint32_t pgd_mix(uint32_t u) {
    u ^= u >> 16; u *= 0x7feb352du; u ^= u >> 15; u *= 0x846ca68bu; u ^= u >> 16;
    return u;
}
__device__ inline float pgd_start_value(float x0, uint32_t row_key, uint32_t c, int random, float eps, float lo, float hi) {
#pragma clang fp contract(off)
    float v = x0;
    if (random) {
        const uint32_t h = pgd_mix(row_key + 0x9E3779B9u * c);
        const float u = (float)(h >> 8) * 0x1p-23f - 1.f;
        const float t = eps * u;
        v = x0 + t;
    }
    return fminf(fmaxf(v, lo), hi);
}
static __global__ __launch_bounds__(256) void pgd_start_kernel(PgdStartParams p) {
    const int m4 = p.M / 4;
    const int64_t total = (int64_t)p.rows_pad * m4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int b = (int)(i / m4);
        const int col = 4 * (int)(i - (int64_t)b * m4);
        f32x4 o = {0.f, 0.f, 0.f, 0.f};
        if (b < p.rows) {
            const uint32_t R = p.idx ? (uint32_t)p.idx[b] : p.row0 + (uint32_t)b;
            const size_t origin = p.idx ? (size_t)p.idx[b] : (size_t)b;
            const f32x4 x0 = *reinterpret_cast<const f32x4 *>(p.X0 + origin * p.ldx0 + col);
            const uint32_t row_key = pgd_mix(pgd_mix(pgd_mix(p.seed) + p.n) ^ R);
#pragma unroll
            for (int r = 0; r < 4; r++)
                o[r] = col + r < p.m_true ? pgd_start_value(x0[r], row_key, (uint32_t)(col + r), p.random, p.eps, p.lo, p.hi) : 0.f;
        }
        *reinterpret_cast<f32x4 *>(p.out + (size_t)b * p.ldo + col) = o;
    }
}

// Integrated gradients (input_grad.hip: gnn_mlp_integrated_gradients_set_range): one of m path points per launch, the step's
// bookkeeping as the epilogue of the same product.  x0 is the ORIGIN row (the resident rows), bl the baseline, `a` the staging
// point the gradient was taken at (g.A0), g formed exactly as above.  In f32, every operation rounded on its own:
//   d = x0 - bl;   S_0 = g(a_0),  S_k = S_{k-1} + g(a_k);   a_{k+1} = bl + alpha_{k+1} * d;   IG = d * (S_{m-1} / m_f)
// Step k < m - 1 stores S_k into S and a_{k+1} into the staging rows (`A`, the buffer g.A0 names); the last step stores IG into
// g.GX.  S is not read at k == 0: what an earlier block or call left there cannot leak.
struct IntGradParams {
    InputGradParams g;         // g.A0: the path point a_k; g.GX / ldg: the attribution (written by the last step only)
    float *A;                  // the staging rows again, to write a_{k+1} (leading dimension g.lda)
    const float *X0; int ldx0; // the origin rows (never written)
    float *S; int lds;         // the running sum, pad(rows) x M
    int k, m;
    float alpha_next, bl, mf;  // alpha_{k+1}, the baseline, (float)m
};
__device__ inline float intgrad_sum(float acc, float fprime, float s_prev, bool first) {
#pragma clang fp contract(off) // (the product is input_grad_kernel's g, rounded before it is added)
    const float g = acc * fprime;
    return first ? g : s_prev + g;
}
__device__ inline float intgrad_point(float x0, float bl, float alpha) {
#pragma clang fp contract(off)
    const float d = x0 - bl;
    const float t = alpha * d;
    return bl + t;
}
__device__ inline float intgrad_value(float x0, float bl, float s, float mf) {
#pragma clang fp contract(off)
    const float d = x0 - bl;
    const float mean = s / mf;
    return d * mean;
}
// grid as input_grad_kernel's.  In place is safe for fgsm_kernel's reason: a lane reads its own four cells of A0, of the origin
// and of S before it stores the same four cells of S and of the staging rows.  Rows >= `rows` and columns >= m_true of every
// buffer a step writes become exact zeros.
template <bool BF>
static __global__ __launch_bounds__(IG_WAVES * 64) void intgrad_kernel(IntGradParams q) {
    const InputGradParams &p = q.g;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int i0 = (blockIdx.x * IG_WAVES + wave) * 16, b0 = blockIdx.y * 16;
    if (i0 >= p.M) return; // (no barrier below)
    const f32x4 acc = ig_tile_product<BF>(p, i0, b0, fr, fq);
    const int b = b0 + fr, col = i0 + 4 * fq;
    const bool first = q.k == 0, last = q.k == q.m - 1;
    f32x4 s = {0.f, 0.f, 0.f, 0.f}, o = {0.f, 0.f, 0.f, 0.f};
    if (b < p.rows) {
        const f32x4 a = *reinterpret_cast<const f32x4 *>(p.A0 + (size_t)b * p.lda + col);
        const f32x4 x0 = *reinterpret_cast<const f32x4 *>(q.X0 + (size_t)b * q.ldx0 + col);
        f32x4 sp = {0.f, 0.f, 0.f, 0.f};
        if (!first) sp = *reinterpret_cast<const f32x4 *>(q.S + (size_t)b * q.lds + col);
#pragma unroll
        for (int r = 0; r < 4; r++) {
            if (col + r >= p.m_true) continue;
            s[r] = intgrad_sum(acc[r], act_prime_from_a(p.act, a[r]), sp[r], first);
            o[r] = last ? intgrad_value(x0[r], q.bl, s[r], q.mf) : intgrad_point(x0[r], q.bl, q.alpha_next);
        }
    }
    if (last) {
        *reinterpret_cast<f32x4 *>(p.GX + (size_t)b * p.ldg + col) = o;
    } else {
        *reinterpret_cast<f32x4 *>(q.S + (size_t)b * q.lds + col) = s;
        *reinterpret_cast<f32x4 *>(q.A + (size_t)b * p.lda + col) = o;
    }
}

// A path point, element-wise, 16 B per lane over the pad(rows) x M staging rows: a = bl + alpha * (x0 - bl) (intgrad_point), the
// first point a_0 -- or, alpha == 0, the baseline rows themselves (bl + 0 * d is bl for every finite d).  Padding: exact zeros.
struct IntGradStartParams {
    const float *X0; int ldx0;
    float *out; int ldo;
    int M, m_true, rows, rows_pad;
    float alpha, bl;
};
static __global__ __launch_bounds__(256) void intgrad_start_kernel(IntGradStartParams p) {
    const int m4 = p.M / 4;
    const int64_t total = (int64_t)p.rows_pad * m4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int b = (int)(i / m4);
        const int col = 4 * (int)(i - (int64_t)b * m4);
        f32x4 o = {0.f, 0.f, 0.f, 0.f};
        if (b < p.rows) {
            const f32x4 x0 = *reinterpret_cast<const f32x4 *>(p.X0 + (size_t)b * p.ldx0 + col);
#pragma unroll
            for (int r = 0; r < 4; r++) o[r] = col + r < p.m_true ? intgrad_point(x0[r], p.bl, p.alpha) : 0.f;
        }
        *reinterpret_cast<f32x4 *>(p.out + (size_t)b * p.ldo + col) = o;
    }
}

// The completeness check: delta[r] = sum_i IG[r][i] - (L_x[r] - L_b[r]), one thread per live row, the row's cells summed in fp64
// in column order (no atomics: the same bits on every run).  L_x / L_b: the per-row losses of the rows and of the baseline rows.
struct IntGradDeltaParams {
    const float *IG; int ldg;
    int d0, rows;
    const float *Lx, *Lb;
    double *delta;
};
static __global__ __launch_bounds__(64) void intgrad_delta_kernel(IntGradDeltaParams p) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= p.rows) return;
    const float *row = p.IG + (size_t)r * p.ldg;
    double sum = 0.0;
    for (int i = 0; i < p.d0; i++) sum += (double)row[i];
    p.delta[r] = sum - ((double)p.Lx[r] - (double)p.Lb[r]);
}

constexpr int SAL_NT = 256;
constexpr int SAL_FLIGHT = 32; // rows a thread has loaded ahead of its sum (a divisor of SAL_NT)
struct SaliencyParams {
    const float *GX; int ldg; // the block's gradient rows
    int d0, rows, n_out;
    const float *Y; int ldy;  // expected rows of the block
    double *sal;                    // [n_out][d0], may be null
    unsigned long long *class_rows; // [n_out], may be null
};

// grid: (ceil(d0 / SAL_NT), n_out)
static __global__ __launch_bounds__(SAL_NT) void saliency_kernel(SaliencyParams p) {
    __shared__ int cls[SAL_NT];
    const int t = threadIdx.x, i = blockIdx.x * SAL_NT + t, c = blockIdx.y;
    const bool own = p.sal && i < p.d0;
    const bool counts = p.class_rows && blockIdx.x == 0 && t == 0;
    double acc = own ? p.sal[(size_t)c * p.d0 + i] : 0.0;
    unsigned long long cnt = 0;
    const float *gx = p.GX + (own ? i : 0);
    for (int r0 = 0; r0 < p.rows; r0 += SAL_NT) {
        __syncthreads();
        cls[t] = r0 + t < p.rows ? expected_class(p.Y + (size_t)(r0 + t) * p.ldy, p.n_out) : -1;
        __syncthreads();
        const int m = p.rows - r0 < SAL_NT ? p.rows - r0 : SAL_NT;
        if (own) {
            // every row is loaded and the other classes' rows add 0.0 (exact: acc >= 0), so the loads do not wait for the sum:
            // SAL_FLIGHT of them are in flight at once (the walk is bound by their latency, one L2 round trip per batch)
            // (rows past the block's end: the last row again, loaded without a branch and added as 0.0 -- their class is -1)
            for (int j0 = 0; j0 < m; j0 += SAL_FLIGHT) {
                float v[SAL_FLIGHT];
#pragma unroll
                for (int u = 0; u < SAL_FLIGHT; u++) v[u] = gx[(size_t)(r0 + (j0 + u < m ? j0 + u : m - 1)) * p.ldg];
#pragma unroll
                for (int u = 0; u < SAL_FLIGHT; u++) acc += cls[j0 + u] == c ? (double)fabsf(v[u]) : 0.0;
            }
        }
        if (counts) for (int j = 0; j < m; j++) cnt += cls[j] == c ? 1ull : 0ull;
    }
    if (own) p.sal[(size_t)c * p.d0 + i] = acc;
    if (counts) p.class_rows[c] += cnt;
}

struct InputGradCombineParams {
    const float *gx[IG_GROUP_MAX]; // member k's gradient rows of the block
    int K;
    float *ens;
    long long n4;                  // float4 elements: pad(rows) * ld[0] / 4
};
static __global__ __launch_bounds__(256) void input_grad_combine_kernel(InputGradCombineParams p) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.n4) return;
    const float kf = (float)p.K;
    f32x4 s = reinterpret_cast<const f32x4 *>(p.gx[0])[i];
#pragma unroll
    for (int k = 1; k < IG_GROUP_MAX; k++) // (unrolled: the table is read with constant offsets into the arguments)
        if (k < p.K) s += reinterpret_cast<const f32x4 *>(p.gx[k])[i];
    f32x4 o;
#pragma unroll
    for (int r = 0; r < 4; r++) o[r] = s[r] / kf;
    reinterpret_cast<f32x4 *>(p.ens)[i] = o;
}

} // namespace gnn
