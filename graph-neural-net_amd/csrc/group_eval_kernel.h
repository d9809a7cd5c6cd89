// group_eval_kernel.h -- EVALUATION of a group of nets of one shape (group.hip) over rows of the group's data set:
//   group_forward_kernel   grid (row tiles) x (members, blockIdx.y = k): one workgroup runs the WHOLE net of member k on one
//                          tile of R = 16 * MT rows and writes, per row, the output vector (softmax of SCE:357-376 or last_act
//                          of GNN:215-218), the loss (SCE:213-217 / GNN:236-239) and the `>=` argmax label (MT:166-168);
//   group_combine_kernel   per row: member k's label against the expected class (count_hits_kernel's rule), member k's loss
//                          into fp64 partial sums with one fixed order, the ensemble's mean output (s = out_0; s += out_k in
//                          member order, one division by (float)K) and the reference's argmax of that mean row;
//   group_loss_finish_kernel  adds the workgroups' loss slots in index order.
//   group_curve_sum_kernel    the curve matrix of a group's observed training loop (rows written by the forward kernel's
//                          LOSS_ONLY form) summed row by row in fp64.
//
// The forward kernel.  Layer l+1 = f(A_l . W_l) is a K loop in chunks of KC rows of W_l: a chunk of the member's W_l (and,
// for layer 0, the same K range of the tile's data-set rows) is brought to LDS with 16-B loads -- the next chunk's loads are
// issued before the current one is multiplied -- and every wave multiplies it into the 16-column tiles it owns (tile
// j * 4 + wave, at most GE_MAXT per wave: a layer wider than 384 takes several passes over K), accumulators in registers.  A_1, A_2, ... live in two LDS images used
// in turn, so no activation goes to memory.  f32 nets: v_mfma_f32_16x16x4_f32, one k-ordered chain per output element;
// bf16 nets: v_mfma_f32_16x16x32_bf16 on the shadows (Wb, DXb), f32 accumulation, activations rounded (RNE) when they become
// the next operand, the output rule from the unrounded sums (gemm_bf16.h's contract).  What a row gets from THIS kernel depends
// on nothing but the row -- not on its place in a tile, a block or the range: rows past the end of the block are staged as zeros
// (never read) and never written.  (Which form a call takes is the host's choice, group_eval.hip: kGroupedMaxBlockRowsF32.)
// Member k's weights are member 0's + k * S bytes (group_kernels.h: the arena rule); the data set is the group's one copy.
#pragma once
#include "gemm_bf16.h"
#include "fused_kernels.h"
#ifndef __HIPCC_RTC__
#include <cstddef>
#include <type_traits>
#endif

namespace gnn {

constexpr int GE_NT = 256;   // four waves
constexpr int GE_MAXT = 6;   // 16-column tiles a wave owns at a time: a pass over 384 columns of a layer (wider layers: more passes)
constexpr int GE_MAXW = 6;   // 16-B pieces of a weight chunk per thread (KC rows x 384 columns)
constexpr int GE_KC_F32 = 16, GE_KC_BF16 = 32;
constexpr int GE_GROUP_MAX = 16; // (= GROUP_MAX of group_kernels.h)

struct GroupEvalParams {
    const void *X;               // first row of the block: DX (f32) or DXb (bf16), leading dimension ld[0]
    const float *Y; int ldy;     // expected rows of the block
    unsigned loss_stride;        // LOSS_ONLY: floats between members in `loss`, there a row [K][loss_stride] of the curve matrix (outside
                                 // the arena).  In the four bytes that padded ldy: every other argument stays where it was.
    const void *W;               // member 0's W (f32) or Wb (bf16), the flat padded buffer
    unsigned long long S;        // bytes between members (the arena rule)
    float *out; float *loss; int32_t *label; // member 0's part of the workspace: [rows][16], [rows], [rows]
    unsigned long long ws_stride;            // 4-byte words between members in the workspace
    int rows;                    // live rows of the block
    int L;
    int d[MAX_LAYERS], ld[MAX_LAYERS];
    unsigned w_off[MAX_LAYERS];  // W_l in the flat buffer (elements)
    int inner_act, last_act, out_kind;
    // LDS (byte offsets; strides in elements): the two activation images, the weight chunk, the layer-0 row chunk, the last sums
    int off_img[2], ldi[2], off_w, off_x, off_z;
};

static_assert(offsetof(GroupEvalParams, loss_stride) == 20 && offsetof(GroupEvalParams, W) == 24, "loss_stride fills ldy's padding");

// host + device: what the kernel needs in LDS for a net, and whether it applies at all (GroupEvalPlan, group_eval.hip)
struct GroupEvalLds { int off_img[2], ldi[2], off_w, off_x, off_z, bytes; bool ok; };
__host__ __device__ constexpr int ge_w_stride(int N, bool bf) {
    // f32 [k][n] image: 16 (mod 32) floats, the four k rows of a fragment read hit disjoint banks (kernels.h);
    // bf16 k-major image read with ds_read_b64_tr_b16: 32 * odd bytes (gemm_bf16.h)
    return bf ? N + ((N / 16) % 2 == 0 ? 16 : 0) : N + (N % 32 == 0 ? 16 : 0);
}
__host__ __device__ constexpr GroupEvalLds ge_lds(const int *ld, int L, bool bf, int mt) {
    GroupEvalLds m{};
    m.ok = false;
    if (L < 3 || L > MAX_LAYERS) return m;
    const int R = 16 * mt, KC = bf ? GE_KC_BF16 : GE_KC_F32, es = bf ? 2 : 4;
    if (ld[L - 1] != 16 || ld[0] > 1024) return m; // the output rule's row; the data-set rows' K loop
    int wmax[2] = {0, 0}, nmax = 0;
    for (int l = 1; l < L - 1; l++) {
        if (ld[l] > 1024) return m;
        if (ld[l] > wmax[(l - 1) & 1]) wmax[(l - 1) & 1] = ld[l];
    }
    for (int l = 1; l < L; l++) if (ld[l] > nmax) nmax = ld[l];
    if (nmax > 64 * GE_MAXT) nmax = 64 * GE_MAXT; // (a pass's columns)
    int off = 0;
    for (int i = 0; i < 2; i++) {
        // f32: row stride 4 (mod 16) floats; bf16: whole 32-k blocks, row stride 8 banks (mod 16) for the b128 fragment reads
        m.ldi[i] = bf ? (wmax[i] + 31) / 32 * 32 + 16 : wmax[i] + 4;
        m.off_img[i] = off;
        off += (wmax[i] ? R * m.ldi[i] * es : 0);
        off = (off + 15) / 16 * 16;
    }
    m.off_w = off; off += KC * ge_w_stride(nmax, bf) * es; off = (off + 15) / 16 * 16;
    m.off_x = off; off += R * (bf ? KC + 16 : KC + 4) * es; off = (off + 15) / 16 * 16;
    m.off_z = off; off += R * 17 * 4;
    m.bytes = off;
    m.ok = off <= 160 * 1024;
    return m;
}

// LOSS_ONLY: the validation form (the observed training loop of a group, group_eval.hip) -- the same sums and, per row, the
// same loss expressions, written to loss[member * loss_stride + row]; no output row, no label.
template <int MT, bool BF, bool LOSS_ONLY = false>
__global__ __launch_bounds__(GE_NT) void group_forward_kernel(GroupEvalParams p) {
    typedef typename std::conditional<BF, __bf16, float>::type T;
    typedef typename std::conditional<BF, bf16x8, float4>::type V16; // one 16-B piece
    constexpr int R = 16 * MT, KC = BF ? GE_KC_BF16 : GE_KC_F32, EPV = BF ? 8 : 4; // elements per 16-B piece
    constexpr int LDX = BF ? KC + 16 : KC + 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char ge_smem[];
    T *const img0 = reinterpret_cast<T *>(ge_smem + p.off_img[0]), *const img1 = reinterpret_cast<T *>(ge_smem + p.off_img[1]);
    T *const Ws = reinterpret_cast<T *>(ge_smem + p.off_w), *const Xs = reinterpret_cast<T *>(ge_smem + p.off_x);
    float *const Zs = reinterpret_cast<float *>(ge_smem + p.off_z);

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, fr = lane & 15, fq = lane >> 4;
    const int row0 = blockIdx.x * R;
    const unsigned long long member = blockIdx.y;
    const T *const Wm = reinterpret_cast<const T *>(reinterpret_cast<const char *>(p.W) + member * p.S);
    const T *const X = reinterpret_cast<const T *>(p.X);
    const int Lm = p.L - 1;

    for (int l = 0; l < Lm; l++) {
        const int K = p.ld[l], N = p.ld[l + 1], n_true = p.d[l + 1];
        const T *const Wl = Wm + p.w_off[l];
        const T *const Ain = (l & 1) ? img0 : img1; // A_l, l >= 1 (A_1 in image 0)
        const int lda = (l & 1) ? p.ldi[0] : p.ldi[1];
        T *const Aout = (l & 1) ? img1 : img0;      // A_{l+1}
        const int ldo = (l & 1) ? p.ldi[1] : p.ldi[0];
        const int ntiles = N >> 4;
        const int nchunks = (K + KC - 1) / KC;
        // column passes: at most 4 * GE_MAXT tiles each, the tiles dealt evenly to the passes (304 columns: one pass of 20 tiles)
        const int npass = (ntiles + 4 * GE_MAXT - 1) / (4 * GE_MAXT);
        const int tpp = (ntiles + npass - 1) / npass;
        for (int q = 0; q < npass; q++) {
            const int tile0 = q * tpp;
            const int ptiles = (ntiles - tile0 < tpp) ? ntiles - tile0 : tpp; // tiles of this pass
            const int c0 = tile0 * 16, ncols = ptiles * 16;
            const int ldw = ge_w_stride(ncols, BF);
            const int npieces = ncols / EPV;      // 16-B pieces per row of the pass's columns of W_l
            const int wpieces = KC * npieces;     // ... per chunk

            f32x4 acc[GE_MAXT][MT];
#pragma unroll
            for (int j = 0; j < GE_MAXT; j++)
#pragma unroll
                for (int mi = 0; mi < MT; mi++) acc[j][mi] = (f32x4){0.f, 0.f, 0.f, 0.f};

            V16 rw[GE_MAXW], rx;
            auto zero16 = []() { V16 z; __builtin_memset(&z, 0, sizeof(z)); return z; };
            auto load_chunk = [&](int k0) {
#pragma unroll
                for (int i = 0; i < GE_MAXW; i++) {
                    const int idx = t + i * GE_NT;
                    rw[i] = zero16();
                    if (idx < wpieces) {
                        const int kk = idx / npieces, c = idx - kk * npieces;
                        if (k0 + kk < K) rw[i] = *reinterpret_cast<const V16 *>(Wl + (size_t)(k0 + kk) * N + c0 + c * EPV);
                    }
                }
                if (l == 0) { // the tile's rows of the data set, K range [k0, k0 + KC): rows past the block are zeros, never read
                    rx = zero16();
                    constexpr int XP = KC / EPV; // pieces per row
                    if (t < R * XP) {
                        const int r = t / XP, c = t - r * XP;
                        if (row0 + r < p.rows && k0 + c * EPV < K)
                            rx = *reinterpret_cast<const V16 *>(X + (size_t)(row0 + r) * K + k0 + c * EPV);
                    }
                }
            };
            auto store_chunk = [&]() {
#pragma unroll
                for (int i = 0; i < GE_MAXW; i++) {
                    const int idx = t + i * GE_NT;
                    if (idx < wpieces) {
                        const int kk = idx / npieces, c = idx - kk * npieces;
                        int row = kk;
                        if constexpr (BF) { // rows permuted inside the 32-k block: the transpose reads then deliver k = 8 g + e (gemm_bf16.h)
                            const int e = kk & 7, g = (kk >> 3) & 3;
                            row = 4 * g + (e & 3) + 16 * (e >> 2);
                        }
                        *reinterpret_cast<V16 *>(Ws + row * ldw + c * EPV) = rw[i];
                    }
                }
                if (l == 0) {
                    constexpr int XP = KC / EPV;
                    if (t < R * XP) {
                        const int r = t / XP, c = t - r * XP;
                        *reinterpret_cast<V16 *>(Xs + r * LDX + c * EPV) = rx;
                    }
                }
            };
            auto multiply = [&](int k0) {
                const T *const A = (l == 0) ? Xs : Ain + k0;
                const int sa = (l == 0) ? LDX : lda;
#pragma unroll
                for (int j = 0; j < GE_MAXT; j++) {
                    const int tile = j * 4 + wave; // (of the pass)
                    if (tile < ptiles) { // (wave-uniform: every lane of the wave executes the transpose reads)
                        if constexpr (BF) {
                            const bf16x8 b = tr_frag(Ws, ldw, tile * 16, 0, lane);
#pragma unroll
                            for (int mi = 0; mi < MT; mi++) {
                                const bf16x8 a = *reinterpret_cast<const bf16x8 *>(A + (mi * 16 + fr) * sa + 8 * fq);
                                acc[j][mi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[j][mi], 0, 0, 0);
                            }
                        } else {
#pragma unroll
                            for (int kk = 0; kk < KC; kk += 4) {
                                const float b = Ws[(kk + fq) * ldw + tile * 16 + fr];
#pragma unroll
                                for (int mi = 0; mi < MT; mi++) {
                                    const float a = A[(mi * 16 + fr) * sa + kk + fq];
                                    acc[j][mi] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[j][mi], 0, 0, 0);
                                }
                            }
                        }
                    }
                }
            };

            load_chunk(0);
            for (int c = 0; c < nchunks; c++) {
                store_chunk();
                __syncthreads(); // (also: the previous layer's activations are in their image)
                if (c + 1 < nchunks) load_chunk((c + 1) * KC);
                multiply(c * KC);
                __syncthreads();
            }

            // C/D map of the 16x16 MFMA: column fr, rows 4 fq + r
            if (l + 1 < Lm) {
#pragma unroll
                for (int j = 0; j < GE_MAXT; j++) {
                    const int tile = j * 4 + wave;
                    if (tile < ptiles) {
                        const int col = c0 + tile * 16 + fr;
#pragma unroll
                        for (int mi = 0; mi < MT; mi++)
#pragma unroll
                            for (int r = 0; r < 4; r++) {
                                const float v = col < n_true ? act_fn(p.inner_act, acc[j][mi][r]) : 0.f;
                                Aout[(mi * 16 + fq * 4 + r) * ldo + col] = (T)v;
                            }
                    }
                }
            } else if (wave == 0) { // (N == 16: one pass of one tile)
#pragma unroll
                for (int mi = 0; mi < MT; mi++)
#pragma unroll
                    for (int r = 0; r < 4; r++) Zs[(mi * 16 + fq * 4 + r) * 17 + fr] = acc[0][mi][r];
            }
        }
        if (BF && l + 1 < Lm && (N & 16)) // the other half of the last 32-k block: zeros, whatever an earlier, wider layer left there
            for (int i = t; i < R * 16; i += GE_NT) Aout[(i >> 4) * ldo + N + (i & 15)] = (T)0.f;
    }
    __syncthreads();

    // the output rule, one thread per row (at most 16 outputs), from the unrounded f32 sums
    if constexpr (LOSS_ONLY) {
        if (t < R && row0 + t < p.rows) {
            const int row = row0 + t, n = p.d[Lm];
            const float *z = Zs + t * 17;
            const float *y = p.Y + (size_t)row * p.ldy;
            float mx = -__builtin_inff(), l = 0.f;
            if (p.out_kind == 0) {
#pragma unroll
                for (int c = 0; c < 16; c++)
                    if (c < n) {
                        const float v = z[c];
                        if (v >= mx) mx = v;
                    }
                float s = 0.f;
#pragma unroll
                for (int c = 0; c < 16; c++) s += c < n ? __expf(z[c] - mx) : 0.f;
                const float lse = mx + __logf(s);
#pragma unroll
                for (int c = 0; c < 16; c++) {
                    const float yy = c < n ? y[c] : 0.f;
                    if (yy != 0.f) l += yy * (lse - z[c]); // -y ln p (SCE:213-217)
                }
            } else {
#pragma unroll
                for (int c = 0; c < 16; c++)
                    if (c < n) {
                        const float dd = act_fn(p.last_act, z[c]) - y[c];
                        l += 0.5f * dd * dd; // GNN:236-239
                    }
            }
            p.loss[member * (unsigned long long)p.loss_stride + row] = l;
        }
        return;
    }
    if (t < R && row0 + t < p.rows) {
        const int row = row0 + t, n = p.d[Lm];
        const float *z = Zs + t * 17;
        const float *y = p.Y + (size_t)row * p.ldy;
        float o[16];
        float mx = -__builtin_inff(), l = 0.f;
        int best = -1;
        bool has_nan = false;
        if (p.out_kind == 0) {
#pragma unroll
            for (int c = 0; c < 16; c++)
                if (c < n) {
                    const float v = z[c];
                    has_nan |= (v != v); // any NaN logit makes every probability NaN: label 0 (kernels.h)
                    if (v >= mx) { mx = v; best = c; }
                }
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < 16; c++) { o[c] = c < n ? __expf(z[c] - mx) : 0.f; s += o[c]; }
            const float inv = 1.f / s, lse = mx + __logf(s);
#pragma unroll
            for (int c = 0; c < 16; c++) {
                o[c] = c < n ? o[c] * inv : 0.f;
                const float yy = c < n ? y[c] : 0.f;
                if (yy != 0.f) l += yy * (lse - z[c]); // -y ln p (SCE:213-217)
            }
        } else {
#pragma unroll
            for (int c = 0; c < 16; c++) {
                o[c] = 0.f;
                if (c < n) {
                    const float a = act_fn(p.last_act, z[c]);
                    const float dd = a - y[c];
                    l += 0.5f * dd * dd; // GNN:236-239
                    if (c == 0) has_nan = (a != a); // element-wise output: only a NaN at index 0 is sticky
                    if (a >= mx) { mx = a; best = c; }
                    o[c] = a;
                }
            }
        }
        if (has_nan) best = 0;
        const unsigned long long sh = member * p.ws_stride;
        float4 *dst = reinterpret_cast<float4 *>(p.out + sh + (size_t)row * 16);
#pragma unroll
        for (int q = 0; q < 4; q++) dst[q] = make_float4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
        p.loss[sh + row] = l;
        p.label[sh + row] = best;
    }
}

// ---- the members' rows combined --------------------------------------------------------------------------------------------
struct GroupCombineParams {
    const float *out[GE_GROUP_MAX];     // member k's output rows of the block, leading dimension ld_out
    const float *loss[GE_GROUP_MAX];    // ... per-row losses
    const int32_t *label[GE_GROUP_MAX]; // ... `>=` argmax labels
    int K, rows, n_out, ld_out;
    const float *Y; int ldy;            // expected rows of the block
    unsigned long long *hits;           // [K + 1]: the members', then the ensemble's
    double *loss_slots;                 // slot (slot0 + blockIdx.x) * GE_GROUP_MAX + k
    int slot0;
    float *mean_out; int32_t *ens_label; // rows of the block, mean_out with leading dimension n_out (either may be null)
};
static __global__ __launch_bounds__(256) void group_combine_kernel(GroupCombineParams p) {
    __shared__ double part[256];
    const int t = threadIdx.x, row = blockIdx.x * 256 + t;
    const bool live = row < p.rows;
    int expected = 0;
    if (live) {
        const float *y = p.Y + (size_t)row * p.ldy;
        for (int i = 0; i < p.n_out; i++) if (y[i] == 1.f) expected = i; // the LAST index whose expected value is 1 (MT:186-188)
    }
#pragma unroll
    for (int k = 0; k < GE_GROUP_MAX; k++) { // (unrolled: the tables are read with constant offsets into the arguments)
        if (k < p.K) {
            const bool hit = live && p.label[k][row] == expected; // MT:195
            const unsigned long long m = __ballot(hit);
            if ((t & 63) == 0 && m) atomicAdd(p.hits + k, (unsigned long long)__popcll(m));
            part[t] = live ? (double)p.loss[k][row] : 0.0;
            __syncthreads();
            for (int w = 128; w > 0; w >>= 1) { // one fixed order: the same bits every time
                if (t < w) part[t] += part[t + w];
                __syncthreads();
            }
            if (t == 0) p.loss_slots[(size_t)(p.slot0 + blockIdx.x) * GE_GROUP_MAX + k] = part[0];
            __syncthreads();
        }
    }
    // the ensemble: the mean output in f32, member order, and the reference's argmax of it (MT:166-168: `>=` from index 0,
    // so ties go to the highest index, a NaN at index 0 stays and a NaN elsewhere is never chosen)
    bool ens_hit = false;
    if (live) {
        const float kf = (float)p.K;
        float best_v = 0.f;
        int best = 0;
        for (int c = 0; c < p.n_out; c++) {
            float s = p.out[0][(size_t)row * p.ld_out + c];
#pragma unroll
            for (int k = 1; k < GE_GROUP_MAX; k++)
                if (k < p.K) s += p.out[k][(size_t)row * p.ld_out + c];
            const float mean = s / kf;
            if (p.mean_out) p.mean_out[(size_t)row * p.n_out + c] = mean;
            if (c == 0) best_v = mean;
            else if (mean >= best_v) { best_v = mean; best = c; }
        }
        if (p.ens_label) p.ens_label[row] = best;
        ens_hit = best == expected;
    }
    const unsigned long long m = __ballot(ens_hit);
    if ((t & 63) == 0 && m) atomicAdd(p.hits + p.K, (unsigned long long)__popcll(m));
}

// The curve matrix of a group's observed training loop summed: rows[(i * K + k) * stride + r] is the loss of validation row r
// for member k after iteration i; workgroup (i, k) adds the row's `cols` LIVE entries (the pad behind them is never written and
// never read) in fp64 -- a strided partial per thread, then one fixed tree: the same bits every time -- into out[i * K + k].
struct CurveSumParams {
    const float *rows; unsigned long long stride; int cols;
    double *out;
};
static __global__ __launch_bounds__(256) void group_curve_sum_kernel(CurveSumParams p) {
    __shared__ double part[256];
    const size_t slot = (size_t)blockIdx.x * gridDim.y + blockIdx.y;
    const float *r = p.rows + slot * p.stride;
    double s = 0.0;
    for (int i = threadIdx.x; i < p.cols; i += 256) s += (double)r[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) p.out[slot] = part[0];
}

// member k's loss sum: the workgroups' slots in index order
static __global__ __launch_bounds__(64) void group_loss_finish_kernel(const double *slots, int n_slots, int K, double *sums) {
    const int k = threadIdx.x;
    if (k >= K) return;
    double s = 0.0;
    for (int i = 0; i < n_slots; i++) s += slots[(size_t)i * GE_GROUP_MAX + k];
    sums[k] = s;
}

} // namespace gnn
