// confusion_kernel.h -- which classes a net gets wrong: confusion matrices counted on the device during an evaluation pass
// (abi.hip: gnn_mlp_evaluate_range; group_eval.hip: gnn_mlp_group_confusion_range).
//   confusion_kernel   up to CF_MAX_TABLES label tables over the same block of rows -- a lone net's labels, or a group's K <= 16
//                      members' and then the ensemble's -- against the block's expected rows: counts[t][expected][label_t[row]]
//                      += 1 for every live row, row = expected class, column = predicted class.  The expected class is
//                      count_hits_kernel's (eval_kernels.h; MT:186-188), taken once per row for all tables.  A label outside
//                      [0, n_out) is not counted (padded rows carry -1); rows >= `rows` are never read.
// Two forms.  LDS_BINS (n_out <= 16, every net of the grouped evaluation plan): a workgroup covers a fixed chunk of CF_CHUNK
// rows, CF_CHUNK / CF_NT per thread, counts into its own T x 256 32-bit bins in LDS with LDS atomics and, after one barrier,
// adds only its non-zero bins to the 64-bit counters in memory -- 60 000 rows are 30 workgroups and at most T x n_out^2 global
// atomics each.  Otherwise (20, 30, 1024 outputs: the rare form) one 64-bit global atomic per row and table.  All sums are
// integer: the result is exact and the same every run whatever the order.
#pragma once
#include "eval_kernels.h"

namespace gnn {

constexpr int CF_MAX_TABLES = 17; // 16 members (GROUP_MAX) + the ensemble
constexpr int CF_NT = 256;
constexpr int CF_CHUNK = 2048;    // rows per workgroup: eight per thread
constexpr int CF_LDS_OUT = 16;    // the LDS form's widest output layer: bins [t][16][16]

struct ConfusionParams {
    const int32_t *label[CF_MAX_TABLES]; // table t's labels of the block's rows
    int T, rows, n_out;
    const float *Y; int ldy;             // expected rows of the block
    unsigned long long *counts;          // [T][n_out][n_out]
    // optional copy of the first T_copy tables' labels: labels_out[t * out_stride + row_offset + row] (null: none)
    int32_t *labels_out; int T_copy; long long out_stride, row_offset;
};

// the expected class of a row: count_hits_kernel's rule, the LAST index whose expected value is exactly 1, 0 when there is none
__device__ inline int expected_class(const float *y, int n_out) {
    int expected = 0;
    for (int i = 0; i < n_out; i++) if (y[i] == 1.f) expected = i; // MT:186-188
    return expected;
}

template <bool LDS_BINS>
static __global__ __launch_bounds__(CF_NT) void confusion_kernel(ConfusionParams p) {
    extern __shared__ unsigned cf_bins[]; // LDS_BINS: [T][16][16]
    const int t = threadIdx.x;
    if constexpr (LDS_BINS) {
        for (int i = t; i < p.T * 256; i += CF_NT) cf_bins[i] = 0u;
        __syncthreads();
    }
    // the thread's rows row0 + t + j * CF_NT: their expected classes first (-1: past the block), once for all tables
    const int row0 = blockIdx.x * CF_CHUNK + t;
    int expected[CF_CHUNK / CF_NT];
#pragma unroll
    for (int j = 0; j < CF_CHUNK / CF_NT; j++) {
        const int row = row0 + j * CF_NT;
        expected[j] = row < p.rows ? expected_class(p.Y + (size_t)row * p.ldy, p.n_out) : -1;
    }
#pragma unroll 1
    for (int k = 0; k < p.T; k++) { // (k is uniform: the table's address is one scalar load from the arguments)
        const int32_t *const label = p.label[k];
        int32_t *const copy = p.labels_out && k < p.T_copy ? p.labels_out + k * p.out_stride + p.row_offset : nullptr;
        unsigned long long *const counts = p.counts + (size_t)k * p.n_out * p.n_out;
#pragma unroll
        for (int j = 0; j < CF_CHUNK / CF_NT; j++) {
            const int row = row0 + j * CF_NT;
            if (expected[j] < 0) continue;
            const int lab = label[row];
            if (copy) copy[row] = lab;
            if ((unsigned)lab >= (unsigned)p.n_out) continue;
            if constexpr (LDS_BINS) atomicAdd(&cf_bins[k * 256 + expected[j] * CF_LDS_OUT + lab], 1u);
            else atomicAdd(counts + (size_t)expected[j] * p.n_out + lab, 1ull);
        }
    }
    if constexpr (LDS_BINS) {
        __syncthreads();
        for (int i = t; i < p.T * 256; i += CF_NT) {
            const unsigned v = cf_bins[i];
            if (v) { // (a non-zero bin has expected, label < n_out)
                const int k = i >> 8, e = (i >> 4) & 15, l = i & 15;
                atomicAdd(p.counts + ((size_t)k * p.n_out + e) * p.n_out + l, (unsigned long long)v);
            }
        }
    }
}

#ifndef __HIPCC_RTC__
// one launch over the block's rows; the form follows n_out
inline hipError_t launch_confusion(const ConfusionParams &p, hipStream_t stream) {
    const dim3 grid((unsigned)((p.rows + CF_CHUNK - 1) / CF_CHUNK));
    if (p.n_out <= CF_LDS_OUT)
        hipLaunchKernelGGL(confusion_kernel<true>, grid, dim3(CF_NT), sizeof(unsigned) * 256 * (size_t)p.T, stream, p);
    else
        hipLaunchKernelGGL(confusion_kernel<false>, grid, dim3(CF_NT), 0, stream, p);
    return hipGetLastError();
}
#endif

} // namespace gnn
