// keep_best_kernel.h -- "which weights along this run were the best on the held-out set?", decided and kept on the device
// (sampler.hip: gnn_mlp_train_sampled_held_out; group.hip: gnn_mlp_group_train_sampled_held_out).
//
// One launch per POINT of the held-out curve, behind the point's evaluation launches on the same stream, for all K members at
// once (blockIdx.y = member; a lone net is K = 1).  Every workgroup of member k reads the same few words -- point p's (hits, loss
// sum) and record p - 1 of the member's history of the running best (point 0 compares against "none") -- and so takes the same
// decision:
//   GNN_BEST_LOSS   the point's loss is not NaN and (there is no best yet, or it is strictly lower than the best's);
//   GNN_BEST_HITS   there is no best yet, or strictly more hits, or equal hits and a strictly lower loss (a NaN is never lower).
// Ties keep the earlier point.  If the point is the new best, the workgroup copies its slice of the member's flat f32 W (n_pad
// floats: the padding travels as it is) to the member's snapshot buffer: KB_VEC 16-byte loads per thread, all of them issued in
// front of the thread's first store, every address guarded by the exact count (n_pad / 4 vectors: a load past it is clamped to
// the last vector, a store past it is skipped).  Thread 0 of the member's first workgroup writes
// record p: a launch reads record p - 1 and writes record p -- different addresses -- so nothing inside a launch depends on an
// order between workgroups, and launches follow one another on the stream.  No LDS, no atomics, no barrier; every value leaves
// through ordinary stores.
#pragma once
#include "kernels.h"

namespace gnn {

constexpr int KB_GROUP_MAX = 16; // (= GROUP_MAX of group_kernels.h)
constexpr int KB_NT = 256;       // threads per workgroup
constexpr int KB_VEC = 4;        // 16-byte vectors per thread: a workgroup copies KB_NT * KB_VEC * 4 = 4096 floats

struct KeepBestRecord { long long hits; double loss; int at; int pad; }; // the running best behind a point (at = -1: none yet)

struct KeepBestParams {
    const float *W[KB_GROUP_MAX];        // member k's weights
    float *snap[KB_GROUP_MAX];           // ... its snapshot buffer, n_pad floats
    KeepBestRecord *hist[KB_GROUP_MAX];  // ... its history, one record per point
    const unsigned long long *hits;      // the point's hit counters, [K]
    const double *loss;                  // ... and loss sums, [K]
    unsigned n4;                         // n_pad / 4
    int point, rule;
};

__device__ __forceinline__ bool kb_better(int rule, long long hits, double loss, const KeepBestRecord &best) {
    if (rule == 0) return !(loss != loss) && (best.at < 0 || loss < best.loss);
    return best.at < 0 || hits > best.hits || (hits == best.hits && loss < best.loss);
}

// grid: (ceil(n4 / (KB_NT * KB_VEC)), K)
static __global__ __launch_bounds__(KB_NT) void keep_best_kernel(KeepBestParams p) {
    const int k = blockIdx.y;
    const long long hits = (long long)p.hits[k];
    const double loss = p.loss[k];
    KeepBestRecord best{0, 0.0, -1, 0};
    if (p.point > 0) best = p.hist[k][p.point - 1];
    const bool better = kb_better(p.rule, hits, loss, best);
    if (blockIdx.x == 0 && threadIdx.x == 0) p.hist[k][p.point] = better ? KeepBestRecord{hits, loss, p.point, 0} : best;
    if (!better) return;
    const f32x4 *src = reinterpret_cast<const f32x4 *>(p.W[k]);
    f32x4 *dst = reinterpret_cast<f32x4 *>(p.snap[k]);
    const unsigned i0 = blockIdx.x * (KB_NT * KB_VEC) + threadIdx.x;
    // (a load past the end reads the last vector instead -- a clamped address, not a branch: behind a branch per load the
    //  compiler waits for each load before it issues the next)
    const unsigned last = p.n4 - 1;
    f32x4 v[KB_VEC];
#pragma unroll
    for (int j = 0; j < KB_VEC; j++) {
        const unsigned i = i0 + j * KB_NT;
        v[j] = src[i < p.n4 ? i : last];
    }
#pragma unroll
    for (int j = 0; j < KB_VEC; j++) {
        const unsigned i = i0 + j * KB_NT;
        if (i < p.n4) dst[i] = v[j];
    }
}

} // namespace gnn
