// handle.h -- internal: the handle behind gnn_mlp_t, the error convention, and the functions the
// translation units of the library call in each other (abi / plan / launch_* / checkpoint / sampler / dp), the timers' slots
// (timer_slot) and the one launcher of a kernel instance held as a pointer (launch_instance; the instances: instances.h).
// Nothing here is part of the C ABI (include/gnn_mlp.h).
#pragma once
#include "../../include/gnn_mlp.h"
#include "fused_kernels.h"
#include "gemm_bf16.h"
#include "gemm_wavek.h"
#include "middle4_kernel.h"
#include "rowblock_kernel.h"
#include "tile_step_kernel.h"
#include "group_kernels.h"
#include "group_eval_kernel.h"
#include "kernels.h"
#include "eval_kernels.h"
#include "keep_best_kernel.h"
#include "lookahead.h"
#include "group_sizes.h"
#include "timer_slots.h"

#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <exception>
#include <new>
#include <string>
#include <vector>

using TimerClass = gnn::host::TimerSlots<hipEvent_t>;

namespace gnn {
namespace host {
// A group call (group.hip) in progress on member 0: every launch of the two-launch step serves all K members
// (group_kernels.h; member k's buffers at member 0's + k * S).  step / momentum per member, as the caller gave them.
struct GroupLaunch {
    int K = 0;
    const char *arena_lo = nullptr; size_t S = 0;
    const void *rb_fn = nullptr; // the grouped row-block kernel of the net (rb_group_function)
    const void *rb_fn_sized = nullptr; // ... and its sized twin (rb_group_sized_function)
    double step[GROUP_MAX] = {}, momentum[GROUP_MAX] = {};
    const char *idx_lo = nullptr; size_t idx_S = 0; // the device index region of a call with one sampler per member (else 0)
    // One batch size per member (gnn_mlp_group_train_sampled_sizes): member k's live rows in the iteration being stepped and in
    // the announced one, set by the loop before every step (group_sizes.h): the launches are the sized twins' (group_kernels.h).
    // Not sized: member 0's counts hold for all.
    bool sized = false;
    int rows[GROUP_MAX] = {}, next_rows[GROUP_MAX] = {};
    // what member 0's control path decides from "the announced batch has the current batch's size" (plan.hip: rb_next) must hold
    // for EVERY member: false when it fails for one
    bool next_same_rows = true;
};
} // namespace host
} // namespace gnn

namespace gnn {
namespace host {
// A resident set: A_0 = f(x) rows [n + PAD][ld[0]], expected rows [n + PAD][ld[L-1]], the bf16 shadow of the inputs (bf16 handles)
struct ResidentSet { float *X = nullptr, *Y = nullptr; __bf16 *Xb = nullptr; int64_t n = 0; };
} // namespace host
} // namespace gnn

struct gnn_mlp {
    int device = 0;
    int L = 0;                 // layerDims.length
    std::vector<int> dims, ld; // logical / padded widths
    std::vector<size_t> w_off; // offset of W_l in the flat padded buffers
    int64_t n_params = 0;      // unpadded
    int64_t n_pad = 0;         // padded flat length
    int out_kind = 0, inner_act = 0, last_act = 0, loss = 0, dtype = 0;
    int max_batch = 0, cap_rows = 0;
    int time = 0;

    float *W = nullptr, *V = nullptr, *G_own = nullptr, *G = nullptr;
    std::vector<float *> act;   // act[l] = f(z_l), l = 0..L-2 ; act[0] = f(x)
    std::vector<float *> delta; // delta[l] = dE/dz_l, l = 1..L-1
    float *logits = nullptr, *prob = nullptr, *ybuf = nullptr, *lossv = nullptr;
    int32_t *labels = nullptr, *idxbuf = nullptr;
    double *stage_out = nullptr;
    // host batches (gnn_mlp_propagate / _loss / _gradient_step ...): pinned f32 slots the calling thread converts the
    // caller's fp64 rows into and the staging kernel reads across PCIe; a slot is rewritten only after the kernel that
    // read it has finished (its event), so call s+1's conversion overlaps step s's kernels (launch_misc.hip)
    static constexpr int kHostSlots = 3;
    float *pin[kHostSlots] = {nullptr, nullptr, nullptr};
    hipEvent_t pin_done[kHostSlots] = {nullptr, nullptr, nullptr};
    bool pin_busy[kHostSlots] = {false, false, false};
    int pin_next = 0;

    float *DX = nullptr, *DY = nullptr; // device-resident dataset (A_0 = f(x) and y)
    // GNN_DTYPE_BF16 (gemm_bf16.h): bf16 roundings of every GEMM operand, written once by its producer
    __bf16 *Wb = nullptr;               // shadow of W, same padded layout
    std::vector<__bf16 *> actb, deltab; // actb[l] l = 0..L-2, deltab[l] l = 1..L-1
    __bf16 *DXb = nullptr;              // dataset inputs
    int64_t dataset_n = 0;
    // The HELD-OUT set (gnn_mlp_upload_held_out*; MT:159-172 reads it as the test rows): a second resident set of the same layout,
    // read by the evaluation passes only -- no training path names it.  resident_set() below gives either set as one struct.
    gnn::host::ResidentSet held;
    bool shared_held = false; // `held` is member 0's (the group's one copy)
    // gnn_mlp_train_sampled_held_out (keep_best_kernel.h): the weights at the best point so far and the running best's history,
    // ordinary allocations made at the first call (never a slice of a group's arena), kept for later calls
    float *best_W = nullptr; gnn::KeepBestRecord *best_hist = nullptr; int best_hist_cap = 0;

    hipStream_t stream = nullptr, own_stream = nullptr;

    // fused small-net path (fused_kernels.h): plan made once at create
    bool fused = false;
    gnn::GradParams grad{};
    int grad_tiles = 0;
    gnn::GradParams grad64{};      // the same layers cut into 64x64 tiles (grad_update64_kernel), used when grad_tiles is large
    int grad_tiles64 = 0;
    bool mid_generic = false; // middle weights exceed LDS: per-layer GEMMs, fwd_first / grad_update chosen per call (hybrid_choice)
    bool mid4 = false;        // middle4_kernel: every middle weight matrix resident in LDS
    gnn::Mid4Params mid4p{};
    size_t mid4_lds_bytes = 0;
    const void *mid4_fn[3] = {nullptr, nullptr, nullptr}; // forward only / forward + backward / the same with A_1 from K slabs
                                                          // (bf16 nets: only slot 2, the bf16 training kernel)
    hipFunction_t mid4_jit[3] = {nullptr, nullptr, nullptr}; // run-time instantiation (jit.h), preferred when set

    // the TRAINING row-block kernel of the two-launch step (rowblock_kernel.h): f32 nets whose plan fits; else mid4_fn[2]
    bool rb = false;
    gnn::RbParams rbp{};
    size_t rb_lds_bytes = 0;
    const void *rb_fn = nullptr;
    hipFunction_t rb_jit = nullptr; // run-time instantiation (jit.h), preferred when set
    int rb_static = 0;              // 1: rb_fn is a prebuilt static-shape instantiation

    // two-launch step (tile_step_kernel.h): the tile kernel of step s also makes the first-layer K slabs of step s+1
    bool chain = false;
    gnn::TileStepParams tsp{};
    int ts_tiles = 0, ts_tiles0 = 0; // blocks of all layers / of layer 0 alone
    uint32_t *ts_map = nullptr, *ts_map0 = nullptr; // workgroup -> tile of the two grids (make_tile_map), device memory
    bool ts_map_args = false; uint32_t ts_map_words[2][gnn::TS_MAP_ARGS / 2]; // ... and packed for the kernel arguments ([0]: all layers, [1]: layer 0)
    gnn::TileHead ts_head[2] = {{0, 0}, {0, 0}}; // the two words that name the regular slots' tiles without a lookup (make_tile_head; {0, 0}: the plan is not regular), same order
    // the merged map of the training form (make_merged_tile_map: light tiles share a workgroup, no CU runs two), kept beside
    // the map above; packed words only.  ts_merge: it is usable -- one entry per CU at most, the words hold it, single f32 net
    bool ts_merge = false; int ts_merge_tiles = 0; uint32_t ts_merge_words[gnn::TS_MAP_ARGS / 2]; gnn::TileHead ts_merge_head = {0, 0};
    float *slabs = nullptr;
    int n_slabs = 0;
    std::string plan_note;    // why the net is NOT on the two-launch path (empty when it is): gnn_mlp_plan_note
    gnn::host::Lookahead la;  // what the slabs hold, the announced next batch, which staging buffer is current (lookahead.h)
    // contiguous copies of SAMPLED batches (two, used alternately): the tile kernel that forms a sampled batch's slabs also
    // writes the rows it gathered; the next step's gradient product reads them in place of the index-gathered rows
    float *xstage[2] = {nullptr, nullptr}; __bf16 *xstage_b[2] = {nullptr, nullptr};
    int specialization = 0;   // 0 runtime-shape kernels, 1 prebuilt static shape, 2 run-time instantiation
    bool jit_tried = false;
    int steps_seen = 0;       // gradient computations so far: the 16th triggers the specialisation

    // train_range graph: one pass over the dataset's batches captured once, replayed many times
    hipGraphExec_t tr_exec = nullptr;
    hipGraph_t tr_graph = nullptr;
    int64_t tr_first_batch = -1; int tr_B = 0; int64_t tr_nb = 0; double tr_step = 0, tr_mom = 0;
    const float *tr_dx = nullptr;

    // Host batches on the two-launch path (gnn_mlp_gradient_step, the reference's own call shape NNT:83): the UPDATE of a step is
    // deferred into the next call's tile launch, which then also forms the new batch's first-layer sums from the weights it has
    // just written -- three dependent launches per call (staging, tile, row-block) instead of four.  `pend` describes the step
    // whose gradient operands (A_0 in act[0], A_l / delta_l in their buffers) wait for that launch; every other entry point
    // applies it first (check_handle).  act0_alt: the second A_0 buffer (the next batch is staged while the pending one is read).
    struct PendingUpdate { bool on = false; int B = 0; float step_over_b = 0.f, momentum = 0.f; } pend;
    float *act0_alt = nullptr;
    bool env_defer_off = false;  // GNN_MLP_DEFER=0: the update in the call that computed it (four launches; development)

    // Evaluation workspace (f32 nets): forward-only buffers for blocks of MORE rows than max_batch -- evaluation over a data set
    // (gnn_mlp_count_hits_range) and the trainer's validation pass (validate(), NNT:102-113: 601 rows at MNIST's size) then run
    // in blocks of up to kEvalRows rows whatever the handle's max_batch, which is sized for TRAINING batches.  Allocated on first
    // use, grown on demand; EvalScope (plan.hip) swaps the buffers in for the duration of a forward pass.
    static constexpr int kEvalRows = 16384;
    int eval_rows_cap = kEvalRows; // GNN_MLP_EVAL_ROWS (development; 0 = blocks of max_batch as until round 4)
    struct EvalWorkspace {
        int rows = 0;
        std::vector<float *> act;   // act[1..L-2]
        float *logits = nullptr, *prob = nullptr, *lossv = nullptr;
        int32_t *labels = nullptr;
    } evalws;
    // the input gradient of the block last run through input_grad.hip: pad(max_batch) x ld[0], made on first use, never a slice
    // of a group's arena
    float *gx = nullptr;
    // the running sum of integrated gradients (intgrad_kernel): the same shape, made on first use, freed where gx is
    float *gsum = nullptr;

    // one process per GPU with the exchange inside the library's step loop (gnn_mlp_rccl_*, dp.hip): this rank's communicator
    void *rccl_comm = nullptr; int rccl_ranks = 0, rccl_rank = 0;

    // member of a group of nets (group.hip): borrowed -- gnn_mlp_destroy, the dataset uploads and gnn_mlp_set_stream refuse it
    gnn_mlp_group *group = nullptr;
    const gnn::host::GroupLaunch *grp = nullptr; // set on member 0 while a group call steps every member (launch_small.hip)
    char *arena_lo = nullptr; size_t arena_bytes = 0; // this handle's slice of the group's arena: never freed by the handle
    bool shared_dataset = false; // DX / DY / DXb are member 0's (the group's one copy)
    bool shared_stream = false;  // own_stream is the group's
    bool dp_replica = false;     // a replica of a gnn_mlp_dp_t (dp.hip): borrowed, its resident rows are the data-parallel handle's

    hipError_t launch_error = hipSuccess; // first refused launch of a module / function-pointer kernel since the last check
    const int32_t *cur_idx = nullptr; // device row indices of the batch being stepped (fused path reads rows through them)

    bool timing = false;
    TimerClass timers[5];

    // development / test switches, read ONCE at create (never on the step path)
    int env_path = 0;          // GNN_MLP_PATH: 0 default, 1 "generic", 2 "nomid4"
    int env_hybrid = -1;       // GNN_MLP_HYBRID: -1 unset, else bit 0 = fwd_first, bit 1 = grad_update
    bool env_tail_off = false; // GNN_MLP_TAIL=0: the three-launch form instead of tail_kernel
    bool env_f32_dma_off = false;  // GNN_MLP_F32_DMA=0: gemm_f32_kernel for every shape (development)
    bool env_bf16_group_off = false; // GNN_MLP_BF16_GROUP=0: one launch per layer's gradient (+ update) product (development)
    bool env_bf16_dma_off = false; // GNN_MLP_BF16_DMA=0: the register-staged bf16 GEMM for every shape (development)
    bool env_wavek_off = false; // GNN_MLP_WAVEK=0: gemm_f32_kernel<32, 32> instead of the wave-K kernel (development)
    bool env_graph = false;    // GNN_MLP_GRAPH=1: train_range replays a captured pass
    bool env_jit_off = false;  // GNN_MLP_JIT=0
    bool env_static_off = false; // GNN_MLP_STATIC=0
    bool env_chain_off = false;  // GNN_MLP_CHAIN=0: three launches per step (fwd_first / middle4 / grad_update)
    int first_wavek_rows = 256;  // launch_fwd_first: blocks of at least this many rows take the (ragged) wave-K GEMM (GNN_MLP_FIRST_WAVEK_ROWS; 0 = never)
    int first_gemm_rows = 2048;  // launch_fwd_first: blocks of at least this many rows take gemm_f32_kernel (GNN_MLP_FIRST_GEMM_ROWS; 0 = never)
    bool env_tile_merge_off = false; // GNN_MLP_TILE_MERGE=0: the tile kernel's training launch on the one-tile-per-workgroup map and kernel, as before the merged map
    bool env_tile_head_off = false; // GNN_MLP_TILE_HEAD=0: the tile kernel's earlier prologue -- every argument from the struct, every tile from the lookup, W and V requested at the top
    bool env_rb_off = false;     // GNN_MLP_ROWBLOCK=0: middle4_kernel<.., SLABS> as the two-launch step's row-block kernel (round 2's form)
};

// A group of nets of one shape (group.hip; evaluation: group_eval.hip)
struct gnn_mlp_group {
    int K = 0, device = 0;
    hipStream_t stream = nullptr;
    char *arena = nullptr;
    size_t S = 0;                 // bytes per member (a multiple of 256)
    std::vector<gnn_mlp *> m;
    bool grouped = false;         // every launch of a step serves all members
    const void *rb_fn = nullptr;  // the grouped row-block kernel (rb_group_function)
    const void *rb_fn_sized = nullptr; // its sized twin (rb_group_sized_function)
    // evaluation in grouped launches (group_eval_kernel.h): the plan made at create, and the workspace -- K x block rows x
    // (16 + 2) words, allocated on first use, grown on demand
    struct EvalPlan { bool ok = false; int mt = 0; gnn::GroupEvalLds lds{}; const void *fn = nullptr, *fn_loss = nullptr; } eval_plan; // (fn_loss: the LOSS_ONLY twin)
    float *eval_ws = nullptr;
    int eval_ws_rows = 0;
    // gnn_mlp_group_train_sampled_held_out: [P][2K + 1] point results (K hit counters, the ensemble's, K loss sums) and the loss
    // slots of one point's combine launches, made at the first call, grown on demand
    char *held_res = nullptr; size_t held_res_bytes = 0;
    int64_t each_grouped = 0, each_mixed = 0; // of the last gnn_mlp_group_train_sampled_each / _sizes call: iterations by grouped launches / member after member
    gnn::host::GroupSizes sizes;  // member k's sizes of the batches member 0's look-ahead state names (group_sizes.h)
};

namespace gnn {
namespace host {

// ---- group_eval.hip ------------------------------------------------------------------------------
// gnn_mlp_group_evaluate_set_range's passes for the held-out curve (group.hip), enqueued only: rows [0, n) of the held-out set,
// the K + 1 hit counters to d_hits (zeroed by the caller), the K loss sums to d_sums, through d_slots (group_point_slots(g, n) doubles)
int group_point_slots(const gnn_mlp_group *g, int64_t n);
int prepare_group_point(gnn_mlp_group *g, int64_t n); // the workspaces a point needs, made before the first step
int enqueue_group_point(gnn_mlp_group *g, int64_t n, unsigned long long *d_hits, double *d_sums, double *d_slots);
void plan_group_eval(gnn_mlp_group *g); // at create: does group_forward_kernel apply to the group's net?
void free_group_eval(gnn_mlp_group *g);
// The validation pass of a group's observed training loop (needs eval_plan.ok; enqueues on member 0's stream, allocates nothing,
// waits for nothing): every member's per-row losses of dataset rows [0, n) to loss_rows[k * stride + row] ...
int enqueue_group_validation(gnn_mlp_group *g, int n, float *loss_rows, int64_t stride);
// ... and n_rows x K such rows summed: d_out[i * K + k] = the fp64 sum of the first n entries of row (i, k)
int enqueue_group_curve_sum(gnn_mlp_group *g, const float *rows, int n_rows, int64_t stride, int n, double *d_out);
// gnn_mlp_group_distill_range's pass (distill.hip), synchronous: rows [first, first + n) of `rs` -- another handle's resident set --
// through gnn_mlp_group_ensemble_range's launches, and behind every block's combine launch the mean rows blended into the
// expected rows y_rows (row `first` of rs.Y; distill_kernel.h).  The caller has checked everything.
int group_distill_rows(gnn_mlp_group *g, const ResidentSet &rs, int64_t first, int64_t n, float *y_rows, float keep);

// ---- error convention (abi.hip) ---------------------------------------------------------------
int fail(int code, const std::string &msg);   // records the calling thread's message, returns `code`
const char *last_error_message();
int check_launches(gnn_mlp *h);
int check_handle(gnn_mlp *h, bool apply_pending = true); // (apply_pending: a host-batch step's deferred update runs first, plan.hip)
int check_batch(const gnn_mlp *h, int B);
int check_range(const gnn_mlp *h, int64_t first, int B);
int check_step_args(gnn_mlp *h, int B, double step, int noise);
int get_flat(gnn_mlp *h, const float *dev, double *flat);
void unpack_params(const gnn_mlp *h, const std::vector<float> &in, double *flat);
// the training set or the held-out set of a handle (GNN_SET_*), as the evaluation passes read them
inline ResidentSet resident_set(const gnn_mlp *h, int set) {
    return set == GNN_SET_HELD_OUT ? h->held : ResidentSet{h->DX, h->DY, h->DXb, h->dataset_n};
}
// what an upload (and gnn_mlp_set_targets_range) on a member of a group is refused with
inline const char *member_set_message(int set) {
    return set == GNN_SET_HELD_OUT ? "a member of a group sees the group's held-out set (gnn_mlp_group_upload_held_out)"
                                   : "a member of a group trains on the group's dataset (gnn_mlp_group_upload_dataset)";
}
// ... and the status for a `set` that is neither, a set never uploaded, rows outside it
int check_set_rows(const gnn_mlp *h, int set, int64_t first, int64_t n);
// gnn_mlp_evaluate_set_range's block loop, enqueued only (abi.hip): hits and the loss sum of rows [first, first + n) of `rs` into
// *d_hits / *d_loss (device; d_hits zeroed by the caller), the confusion launch when cf_counts is given
int enqueue_evaluation(gnn_mlp *h, const ResidentSet &rs, int64_t first, int64_t n, unsigned long long *d_hits, double *d_loss,
                       unsigned long long *cf_counts, int32_t *labels_out);
int set_flat(gnn_mlp *h, float *dev, const double *flat);

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return ::gnn::host::fail(GNN_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)
#define TRY_LAUNCHES(h)                              \
    do {                                             \
        int rc_ = ::gnn::host::check_launches(h);    \
        if (rc_ != GNN_OK) return rc_;               \
    } while (0)
#define TRY(expr)                      \
    do {                               \
        int rc_ = (expr);              \
        if (rc_ != GNN_OK) return rc_; \
    } while (0)

// Every entry point of the C ABI runs its body through this: the header promises that nothing throws or aborts
// across the boundary (a JVM caller would be taken down by std::terminate), and the bodies use std::vector,
// std::string, std::thread and new.  An exception becomes a status + message like any other failure.
int fail_from_exception(const char *what) noexcept;
template <class F> int guarded(F &&body) noexcept {
    try {
        return body();
    } catch (const std::bad_alloc &) {
        return fail_from_exception("out of host memory");
    } catch (const std::exception &e) {
        return fail_from_exception(e.what());
    } catch (...) {
        return fail_from_exception("unknown C++ exception");
    }
}

inline int grid_for(int64_t n) {
    int64_t b = (n + 255) / 256;
    if (b < 1) b = 1;
    if (b > 2048) b = 2048;
    return (int)b;
}

// ---- timing and launches ----------------------------------------------------------------
// the next timer slot of class `cls` (timer_slots.h): false when timing is off, cls < 0 (or past the last class), the class is full or an event cannot be created
inline bool timer_slot(gnn_mlp *h, int cls, hipEvent_t *ev0, hipEvent_t *ev1) {
    return take_timer_slot(h->timing, h->timers, cls, [](hipEvent_t *e) { return hipEventCreate(e) == hipSuccess; }, ev0, ev1);
}

struct ScopedTimer { // events recorded around a stretch of the stream
    gnn_mlp *h; hipEvent_t ev0 = nullptr, ev1 = nullptr; bool on;
    ScopedTimer(gnn_mlp *h_, int cls) : h(h_), on(timer_slot(h_, cls, &ev0, &ev1)) {
        if (on) (void)hipEventRecord(ev0, h->stream);
    }
    ~ScopedTimer() {
        if (on) (void)hipEventRecord(ev1, h->stream);
    }
};

// Launch with the dispatch's OWN begin/end timestamps (hipExtLaunchKernel start/stop events): the
// elapsed time between them is the kernel's execution time, the same quantity rocprofv3's
// kernel trace reports -- unlike events recorded around a launch, which add marker overhead.
template <class K, class... P> void launch_timed(gnn_mlp *h, int cls, K kernel, dim3 grid, dim3 block, size_t lds, const P &...params) {
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    if (timer_slot(h, cls, &ev0, &ev1)) hipExtLaunchKernelGGL(kernel, grid, block, (uint32_t)lds, h->stream, ev0, ev1, 0, params...);
    else hipLaunchKernelGGL(kernel, grid, block, lds, h->stream, params...);
}

// The launch of an instance held as a POINTER (instances.h; `args` as hipLaunchKernel takes them), timed like launch_timed:
// the run-time instantiation `module_fn` when set (jit.h; a module launch gives its global size in threads), else `fn`.
// A refused launch must not pass for a step: the first one since the last check goes to h->launch_error (check_launches);
// a null instance -- a form its family does not have -- is a refused launch.
inline void launch_instance(gnn_mlp *h, int cls, const void *fn, hipFunction_t module_fn, dim3 grid, dim3 block, size_t lds, void **args) {
    if (!fn && !module_fn) { // (before a timer slot is taken: its events would never be recorded)
        if (h->launch_error == hipSuccess) h->launch_error = hipErrorInvalidValue;
        return;
    }
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    const bool timed = timer_slot(h, cls, &ev0, &ev1);
    hipError_t le;
    if (module_fn) le = hipExtModuleLaunchKernel(module_fn, grid.x * block.x, grid.y * block.y, grid.z * block.z, block.x, block.y, block.z, lds, h->stream, args, nullptr, ev0, ev1, 0);
    else if (timed) le = hipExtLaunchKernel(const_cast<void *>(fn), grid, block, args, lds, h->stream, ev0, ev1, 0);
    else le = hipLaunchKernel(fn, grid, block, args, lds, h->stream);
    if (le != hipSuccess && h->launch_error == hipSuccess) h->launch_error = le;
}

// More than 64 KB of dynamic LDS needs hipFuncAttributeMaxDynamicSharedMemorySize -- per kernel AND per device (a handle over N
// devices, dp.hip, launches the same instantiation on each): `done` is the instantiation's own flag array, indexed by the handle's
// device (the handle's device is current when its kernels are launched).
constexpr int kMaxOptInDevices = 64;
template <class K> void opt_in_dynamic_lds(gnn_mlp *h, K kernel, size_t bytes, bool (&done)[kMaxOptInDevices]) {
    const bool tracked = h->device >= 0 && h->device < kMaxOptInDevices;
    if (tracked && done[h->device]) return;
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) {
        if (h->launch_error == hipSuccess) h->launch_error = hipGetLastError();
    }
    if (tracked) done[h->device] = true;
}

// Device allocations of gnn_mlp_create: hipMalloc, or -- while group.hip creates the members of a group -- the next
// 256-byte-aligned slice of the member's part of the group's arena (record: hipMalloc as usual, and count the bytes).
struct ArenaCarve { char *base = nullptr; size_t cap = 0, used = 0; bool record = false; };
extern thread_local ArenaCarve *t_arena;
int dev_bytes(void **p, size_t bytes);
void dev_release(gnn_mlp *h, void *p); // hipFree, except for a slice of the handle's arena

// Zero-filled device allocation.  The fill is enqueued on the HANDLE's stream: that stream is
// non-blocking, so a legacy-stream hipMemset would not be ordered with the kernels that follow.
template <typename T> int dev_alloc(T **p, size_t n, hipStream_t s) {
    TRY(dev_bytes(reinterpret_cast<void **>(p), sizeof(T) * (n ? n : 1)));
    HIP_TRY(hipMemsetAsync(*p, 0, sizeof(T) * (n ? n : 1), s));
    return GNN_OK;
}

// scratch device allocation released on every exit path
struct DevScratch {
    void *p = nullptr;
    ~DevScratch() { if (p) (void)hipFree(p); }
    int alloc(size_t bytes) {
        HIP_TRY(hipMalloc(&p, bytes ? bytes : 1));
        return GNN_OK;
    }
    template <class T> T *as() const { return static_cast<T *>(p); }
};

// ---- launch_gemm.hip: per-layer f32 GEMMs and the three-launch small-net kernels -----------------
int pick_tile(int M, int N);
bool wavek_fits(int M, int N, int K);
void forward(gnn_mlp *h, const float *a0, int B, int first_l = 1, bool stop_before_last = false);
void run_output(gnn_mlp *h, const float *y, int B, bool want_prob, bool want_delta, bool want_loss, bool want_label);
void backward(gnn_mlp *h, const float *a0, int B, bool fused_update, float step_over_b, float momentum,
              bool data_only = false, bool have_last_delta = false);
void launch_fwd_first(gnn_mlp *h, const float *a0, int B);
void fused_gradient(gnn_mlp *h, const float *a0, int B, bool fused_update, float step_over_b, float momentum);
void launch_tail(gnn_mlp *h, const float *a0, const float *y, int B, bool backward, bool want_prob, bool want_loss, bool want_label);

// ---- launch_bf16.hip ---------------------------------------------------------------------------
void forward_bf16(gnn_mlp *h, const __bf16 *a0b, int B, bool stop_before_last = false);
void backward_bf16(gnn_mlp *h, const __bf16 *a0b, int B, bool fused_update, float step_over_b, float momentum, bool have_tail = false);
void to_bf16(gnn_mlp *h, const float *src, __bf16 *dst, size_t n);

// ---- launch_small.hip: the row-block kernel and the tile-owner kernel ----------------------------
// which rows the row-block kernel copies to a staging buffer while its row tail runs (RbParams::xcopy): none, its own
// sampled batch's (to xstage[xstage_cur]), or the announced NEXT sampled batch's (to the other buffer)
enum { RB_COPY_NONE = 0, RB_COPY_CURRENT = 1, RB_COPY_NEXT = 2 };
struct PeerGradients { const float *G[TS_MAX_PEERS]; int n; unsigned slice; }; // gsrc 3 / 4 of launch_tile_step (dp.hip)
void plan_mid4(gnn_mlp *h);
void plan_rowblock(gnn_mlp *h); // (after plan_chain: the kernel exists for the two-launch step only)
void try_specialize(gnn_mlp *h);
int static_shape_of(const gnn_mlp *h);
void fused_forward(gnn_mlp *h, const float *a0, const float *y, int B, bool backward, bool want_prob,
                   bool want_loss, bool want_label, bool from_slabs = false, int copy_rows = RB_COPY_NONE);
void launch_tile_step(gnn_mlp *h, int gsrc, int gdst, const NextBatch *next, const float *a0, int B, float step_over_b, float momentum,
                      bool staged = false, const PeerGradients *peers = nullptr, bool next_staged = false);

// ---- group_kernels.hip / group_kernels_gnn.hip: the grouped instances ----------------------------------
const void *rb_group_function(const gnn_mlp *h); // the grouped row-block kernel of h's net, or null (h->rb must hold)
// the launches of launch_small.hip for every member of h->grp: member 0's arguments, one grid row per member
// (GroupLaunch::sized: the sized twins below)
void launch_tile_step_group(gnn_mlp *h, int gsrc, int gdst, bool fwd, unsigned grid, const TileStepParams &t, int B);
void launch_rowblock_group(gnn_mlp *h, int B, void *const *head_and_params); // (GNN_RB_HEAD_PARAMS + the RbParams)
GroupArgs group_args(const GroupLaunch &g, int nbx, int B, const int *rows);
// ---- group_kernels_sized.hip / group_kernels_sized_gnn.hip: the sized twins (every member with its own row count) --------
const void *rb_group_sized_function(const gnn_mlp *h);
void launch_tile_step_group_sized(gnn_mlp *h, int gsrc, int gdst, bool fwd, unsigned grid, const TileStepParams &t);
void launch_rowblock_group_sized(gnn_mlp *h, void *const *head_and_params);

// ---- sampler.hip ---------------------------------------------------------------------------------
// validate(validation_size) (NNT:102-113) on the device: the summed loss of dataset rows [0, n) into *d_out (fp64, device)
int validation_loss_sum(gnn_mlp *h, int n, double *d_out);
// the same pass with the per-sample losses LEFT in loss_row[0..n) (device; the caller sums rows later): one block, no reduction launch.
// false when the pass needs more than one block (n above the evaluation block size): the caller then takes validation_loss_sum
bool validation_losses_to_row(gnn_mlp *h, int n, float *loss_row, int *rc);

// ---- launch_misc.hip: encodings, gathers, the flat update ---------------------------------------
void launch_convert_rows(gnn_mlp *h, const double *src, int d, float *dst, int ld, int64_t rows, int64_t rows_pad, int act, int apply_act);
void launch_encode_u8(gnn_mlp *h, const uint8_t *pix, int d, float *dst, int ld, int64_t rows, int act);
void launch_onehot_u8(gnn_mlp *h, const uint8_t *lab, int n_classes, float *dst, int ld, int64_t rows);
int stage_batch(gnn_mlp *h, const double *X, const double *Y, int B); // host fp64 rows -> act[0] = f(x), ybuf (Y may be null)
void release_host_staging(gnn_mlp *h);
int export_rows(gnn_mlp *h, const float *src, int ld, int d, int B, double *host_dst);
void launch_gather(gnn_mlp *h, const int32_t *d_idx, int B);
void launch_flat_update(gnn_mlp *h, int B_global, double step, double momentum);

// ---- plan.hip: which kernels a net takes, and one step made of them -------------------------------
void plan_fused(gnn_mlp *h);
void plan_chain(gnn_mlp *h);
const __bf16 *a0_bf16(const gnn_mlp *h, const float *a0);
void ensure_slabs(gnn_mlp *h, const NextBatch &batch);
bool update_by_tiles(gnn_mlp *h, int gsrc, float step_over_b, float momentum, const PeerGradients *peers = nullptr);
void hint_range(gnn_mlp *h, int64_t row0, int B);
void do_forward(gnn_mlp *h, const float *a0, const float *y, int B, bool want_prob, bool want_loss, bool want_label);
void do_gradient(gnn_mlp *h, const float *a0, const float *y, int B, bool fused_update, float step_over_b, float momentum,
                 bool resident = false);
void maybe_specialize(gnn_mlp *h);
// rows a forward-only block may have on this handle: max_batch, or kEvalRows through the evaluation workspace (f32)
int eval_block_rows(const gnn_mlp *h, int64_t rows_wanted);
struct EvalScope { // for blocks above max_batch: the evaluation workspace's buffers stand in for act[1..], logits, prob, lossv, labels
    gnn_mlp *h; bool on = false;
    EvalScope(gnn_mlp *h_, int rows, int *rc);
    ~EvalScope();
    void swap();
};
void free_eval_workspace(gnn_mlp *h);
void free_input_grad(gnn_mlp *h); // (input_grad.hip; destroy_handle calls it)
// input_grad.hip: behind a do_gradient on (a0, B), the launch over delta_1 . W_0^T -- the block's input gradient into h->gx
// (the caller has made it), or with `step` the rows a0 moved along its sign into step->out (input_grad_kernel.h; out == a0 is
// allowed).  The descriptor names the epilogue: origin == null, fgsm_kernel (a0 + eps * sign, clipped); otherwise pgd_kernel, one
// projected step of size alpha around row `idx ? idx[b] : b` of `origin` (resident rows, leading dimension ld[0])
struct AdvStep {
    float eps, lo, hi; float *out;
    float alpha = 0.f; const float *origin = nullptr; const int32_t *idx = nullptr;
};
void enqueue_input_grad(gnn_mlp *h, const float *a0, int B, const AdvStep *step = nullptr);
// the start rows of the projected attack into h->act[0] (pgd_start_kernel): `origin` / `idx` as above, row0 the set index of the
// block's first row (idx == null), n the iteration's number, seed < 0: the origin rows clipped to the box alone
void enqueue_pgd_start(gnn_mlp *h, const AdvStep &step, int B, int64_t row0, int64_t seed, int n);
// adversarial.hip: the nets whose staging rows may be moved on the device -- lone nets (GNN_ERR_STATE for a member of a group or a
// replica) whose inner activation is the identity on non-negative values (GNN_ERR_UNSUPPORTED otherwise: the device holds f(x))
int check_adv_net(const gnn_mlp *h);
void rccl_detach_handle(gnn_mlp *h); // (dp.hip; gnn_mlp_destroy calls it)
bool can_defer_update(const gnn_mlp *h);
int step_on_host_batch_deferred(gnn_mlp *h, int B, double step, double momentum); // act[0] / ybuf hold the staged batch
void flush_pending_update(gnn_mlp *h);
int step_on_rows(gnn_mlp *h, const float *a0, const float *y, int B, double step, double momentum, bool resident);
int step_on_device_indices(gnn_mlp *h, const int32_t *d_idx, int B, double step, double momentum);

// ---- abi.hip / sampler.hip: bodies the group entry points (group.hip) share with the single-net ones --------------------
int create_handle(const int32_t *dims, int n_dims, int out_kind, int inner_act, int last_act, int loss, int64_t seed, int dtype,
                  int device, int max_batch, hipStream_t shared_stream, gnn_mlp **out);
void destroy_handle(gnn_mlp *h);
int upload_dataset_f64(gnn_mlp *h, const double *X, const double *Y, int64_t N, int set = GNN_SET_TRAIN);
int upload_dataset_u8(gnn_mlp *h, const uint8_t *pixels, const uint8_t *labels, int64_t N, int set = GNN_SET_TRAIN);
int train_range_checks(gnn_mlp *h, int64_t first, int B, int n_steps, double step);
int train_range_steps(gnn_mlp *h, int64_t first, int B, int s, int n_steps, double step, double momentum);
int train_sampled_checks(gnn_mlp *h, gnn_sampler_t *s, int iterations, int batch, double step, int noise);
// What the sampled training loop (sampler.hip: train_sampled_run) calls between the steps it enqueues: after_step(i) when step
// i's launches are on the handle's stream, after_chunk(i_end) when every step of a sampler chunk -- iterations up to i_end,
// i_end == iterations for the last one -- is.  A status other than GNN_OK ends the loop.
struct SampledObserver {
    virtual int after_step(int i) = 0;
    virtual int after_chunk(int i_end) { (void)i_end; return GNN_OK; }
    virtual ~SampledObserver() {}
};
// The group's side of the loop with ONE SAMPLER PER MEMBER (group.hip: gnn_mlp_group_train_sampled_each), run on member 0's handle:
// region(lo, slice_bytes) when the device index region exists (member m's ring at lo + m * slice_bytes) and region(null, 0)
// just before it is released; mixed_step(d_idx, counts) steps ONE iteration whose batch sizes counts[m] differ between the
// members -- member m's indices at d_idx[m] -- and leaves member 0's handle ready for the next grouped step.
// sized() (gnn_mlp_group_train_sampled_sizes): the grouped launches take every member's own row count, so NO iteration is
// mixed -- the loop calls step_sizes(rows, next_rows) in front of every step with the members' live rows in the iteration it is
// about to step and in the one it announces (null: none announced), then steps member 0 as ever.
struct SampledEach {
    virtual void region(const int32_t *lo, size_t slice_bytes) = 0;
    virtual int mixed_step(const int32_t *const *d_idx, const int *counts) = 0;
    virtual bool sized() const { return false; }
    virtual void step_sizes(const int *rows, const int *next_rows) { (void)rows; (void)next_rows; }
    virtual ~SampledEach() {}
};
// What steps an iteration INSTEAD of step_on_device_indices (a lone handle's call; adversarial.hip: the batch is perturbed first):
// nothing is announced to the look-ahead state then, the draws, chunks and uploads are the loop's own.
struct SampledStep {
    virtual int step(const int32_t *d_idx, int B) = 0;
    virtual ~SampledStep() {}
};
// The loop itself, for n samplers (a lone handle: &s, 1, &batch, each null).  batches[m]: sampler m's nominal batch size (all
// equal unless each->sized()); every ring has the slot stride of the largest (index_ring.h)
int train_sampled_run(gnn_mlp *h, gnn_sampler_t *const *samplers, int n, int iterations, const int *batches, double step,
                      double momentum, int noise, SampledObserver *obs, SampledEach *each, SampledStep *stepper = nullptr);
// the held-out curve (sampler.hip; keep_best_kernel.h): a handle's snapshot buffer and history for `points` points, the launch for
// K nets of one shape, the arguments both entry points refuse
int ensure_keep_best(gnn_mlp *h, int points);
int launch_keep_best(hipStream_t stream, gnn_mlp *const *m, int K, const unsigned long long *hits, const double *loss, int point, int rule);
int check_held_out_args(const gnn_mlp *h, int every, int64_t held_rows, int rule, const void *point_hits, const void *point_loss,
                        const void *best_point);
gnn_sampler_t *sampler_copy(const gnn_sampler_t *s);
void sampler_assign(gnn_sampler_t *dst, const gnn_sampler_t *src);

} // namespace host
} // namespace gnn
