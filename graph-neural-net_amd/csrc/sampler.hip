// sampler.hip -- the trainer's side of the boundary (NNT:143-168): the exact epoch sampler of NeuralNetTrainer.sample /
// refillSampler on java.util.Random, and gnn_mlp_train_sampled, the train loop of NNT:60-92 on a resident dataset.
#include "handle.h"
#include "java_random.h"
#include "index_ring.h"

#include <algorithm>

using namespace gnn;
using namespace gnn::host;

// The k-th set bit (k 0-based, k < popcount) of a 64-bit word: deposit one bit at the k-th set position, count the zeros below it.
#if defined(__x86_64__)
__attribute__((target("bmi2"))) static inline int select_bit_bmi2(uint64_t w, int k) { return (int)__builtin_ctzll(__builtin_ia32_pdep_di(1ull << k, w)); }
static inline bool have_bmi2() { return __builtin_cpu_supports("bmi2"); }
#else
static inline int select_bit_plain(uint64_t w, int k);
static inline int select_bit_bmi2(uint64_t w, int k) { return select_bit_plain(w, k); }
static inline bool have_bmi2() { return false; }
#endif
static inline int select_bit_plain(uint64_t w, int k) {
    for (; k > 0; k--) w &= w - 1;
    return (int)__builtin_ctzll(w);
}

struct gnn_sampler {
    int32_t master = 0, remaining = 0;
    // "row still in dataSampler" as one bit per row, 64 rows per word, and a Fenwick tree over the words' counts: the r-th
    // remaining row in master order is what ArrayList.get(r) returns after removals (NNT:152-154).  A tree over words, not
    // rows: 938 counters for MNIST's 60 000 rows stay in L1 and the walk is 10 levels instead of 16 through L2 -- the sampler
    // feeds a training loop whose step is 13 us, and at two row-level walks per draw it was the slower of the two
    // (14.3 us per batch of 128 against 13.2; tools/bench_trainer.py).
    std::vector<uint64_t> bits;
    std::vector<int32_t> fen; // 1-based over the words
    int32_t words = 0;
    JavaRandom rnd{1};
    int log2w = 0;
    bool bmi2 = false;
    void refill() { // refillSampler NNT:164-168
        bits.assign((size_t)words, ~0ull);
        if (master % 64) bits[(size_t)words - 1] = (1ull << (master % 64)) - 1;
        // (entries behind the last word, up to the next power of two, read as "more than any k": the walk below needs no bounds test)
        fen.assign(((size_t)2 << log2w) + 1, INT32_MAX);
        std::fill(fen.begin(), fen.begin() + words + 1, 0);
        for (int32_t i = 1; i <= words; i++) {
            fen[i] += (int32_t)__builtin_popcountll(bits[(size_t)i - 1]);
            const int32_t j = i + (i & -i);
            if (j <= words) fen[j] += fen[i];
        }
        remaining = master;
    }
    int32_t take(int32_t r) { // remove and return the r-th (0-based) remaining row
        int32_t pos = 0, k = r + 1;
        for (int32_t pw = 1 << log2w; pw > 0; pw >>= 1) { // (selects, not branches: the comparison is a coin toss per level)
            const int32_t f = fen[pos + pw];
            const bool go = f < k;
            pos += go ? pw : 0;
            k -= go ? f : 0;
        }
        // word `pos` (0-based) holds the row: its (k-1)-th set bit
        const uint64_t w = bits[(size_t)pos];
        const int bit = bmi2 ? select_bit_bmi2(w, k - 1) : select_bit_plain(w, k - 1);
        bits[(size_t)pos] = w & ~(1ull << bit);
        for (int32_t i = pos + 1; i <= words; i += i & -i) fen[i] -= 1;
        remaining--;
        return pos * 64 + bit; // 0-based row
    }
};

extern "C" {

int gnn_sampler_create(int32_t master_size, int64_t seed, gnn_sampler_t **out) { return guarded([&]() -> int {
    if (!out || master_size <= 0) return fail(GNN_ERR_BAD_ARG, "bad sampler arguments");
    gnn_sampler *s = new gnn_sampler();
    s->master = master_size;
    s->words = (master_size + 63) / 64;
    s->rnd.set_seed(seed);
    while ((1 << (s->log2w + 1)) <= s->words) s->log2w++;
    s->bmi2 = have_bmi2();
    s->refill();
    *out = s;
    return GNN_OK;
}); }

int gnn_sampler_destroy(gnn_sampler_t *s) { delete s; return GNN_OK; }

int gnn_sampler_sample(gnn_sampler_t *s, int batch, int32_t *out_idx, int *n_out) { return guarded([&]() -> int {
    if (!s || !out_idx || !n_out || batch <= 0) return fail(GNN_ERR_BAD_ARG, "bad sampler arguments");
    int n = 0, before_refill = 0; // rows drawn before a refill inside this batch: only THEY can come again (within an epoch rows are distinct)
    for (int i = 0; i < batch; i++) {
        if (s->remaining == 0) { s->refill(); before_refill = n; } // NNT:149-151
        const int32_t r = s->rnd.next_int(s->remaining);           // NNT:152
        const int32_t row = s->take(r);                            // NNT:153-154
        bool dup = false;                                          // HashMap.put, NNT:155
        for (int k = 0; k < before_refill; k++) if (out_idx[k] == row) { dup = true; break; }
        if (!dup) out_idx[n++] = row;
    }
    *n_out = n;
    return GNN_OK;
}); }

} // extern "C"

namespace gnn {
namespace host {
// validate(validation_size) of NNT:102-113 without its division: calculateLoss over the first n samples in master order
// (dataset rows [0, n)), block by block on the handle's stream, summed into ONE fp64 slot on the device.
int validation_loss_sum(gnn_mlp *h, int n, double *d_out) {
    const int Lm = h->L - 1;
    const int block = eval_block_rows(h, n); // (601 rows at MNIST's size: ONE block through the evaluation workspace instead of five of max_batch)
    int rc_ws = GNN_OK;
    EvalScope scope(h, block, &rc_ws);
    if (rc_ws != GNN_OK) return rc_ws;
    for (int off = 0; off < n; off += block) {
        const int B = std::min(block, n - off);
        do_forward(h, h->DX + (size_t)off * h->ld[0], h->DY + (size_t)off * h->ld[Lm], B, false, true, false);
        hipLaunchKernelGGL(sum_loss_kernel, dim3(1), dim3(256), 0, h->stream, LossSumParams{h->lossv, B, d_out, off > 0 ? 1 : 0});
    }
    return GNN_OK;
}
bool validation_losses_to_row(gnn_mlp *h, int n, float *loss_row, int *rc) {
    *rc = GNN_OK;
    if (eval_block_rows(h, n) < n) return false;
    const int Lm = h->L - 1;
    EvalScope scope(h, n, rc);
    if (*rc != GNN_OK) return true;
    float *keep = h->lossv;
    h->lossv = loss_row; // (the forward kernels write loss[row]: straight into the matrix's row)
    do_forward(h, h->DX, h->DY, n, false, true, false);
    h->lossv = keep;
    return true;
}
} // namespace host
} // namespace gnn

// The loop NNT:60-92 on a resident dataset.
int gnn::host::train_sampled_checks(gnn_mlp *h, gnn_sampler_t *s, int iterations, int batch, double step, int noise) {
    if (!s) return fail(GNN_ERR_BAD_ARG, "null sampler");
    TRY(check_step_args(h, batch, step, noise));
    if (!h->DX) return fail(GNN_ERR_STATE, "no dataset uploaded");
    if (iterations <= 0) return fail(GNN_ERR_BAD_ARG, "iterations must be positive (NNT:62)");
    if (s->master != h->dataset_n) return fail(GNN_ERR_BAD_ARG, "sampler size differs from the dataset");
    if (batch >= s->master) return fail(GNN_ERR_BAD_ARG, "batchSize must be below the data size (NNT:63)");
    return GNN_OK;
}
// the sampler's whole state: the group's fallback replays one sampler's draws for every member (group.hip)
gnn_sampler_t *gnn::host::sampler_copy(const gnn_sampler_t *s) { return new gnn_sampler(*s); }
void gnn::host::sampler_assign(gnn_sampler_t *dst, const gnn_sampler_t *src) { *dst = *src; }

namespace {
// The index storage of one call of the loop below: n rings of kIndexRingSlots chunk slots on the host and on the device
// (index_ring.h: IndexRingLayout says where everything lies, UploadWindow which chunks are where), slice m of ONE pinned and ONE
// device allocation -- the device one is the index region of group_kernels.h -- and the drawn batch sizes beside them.
// The host ring is PINNED memory and every upload is followed by an event: the copy is then truly asynchronous (from pageable
// memory hipMemcpyAsync stages the data before it returns -- in this runtime by waiting for the stream, i.e. for every step
// queued so far: the GPU idled at each chunk boundary, and the slot's safety rested on that behaviour), and a host slot goes
// back to the samplers only when its event has completed.
struct DeviceIndexRing {
    // an iteration on the device: member 0's indices, every member's batch size, whether those sizes agree
    struct Iteration {
        const int32_t *idx0 = nullptr; int counts[GROUP_MAX]; bool same = true;
        explicit operator bool() const { return idx0 != nullptr; }
    };
    const IndexRingLayout lay; UploadWindow win; hipStream_t stream; SampleRing &sr;
    int32_t *host = nullptr; hipEvent_t ev[kIndexRingSlots] = {};
    std::vector<int> cnt, dcnt; // the batch sizes as drawn (the samplers write them) / of the chunks on the device
    DevScratch dev;
    DeviceIndexRing(const IndexRingLayout &lay_, const ChunkSchedule &sched, hipStream_t stream_, SampleRing &sr_)
        : lay(lay_), win{sched}, stream(stream_), sr(sr_), cnt(lay_.total_counts()), dcnt(lay_.total_counts(), 0) {}
    ~DeviceIndexRing() { if (host) (void)hipHostFree(host); for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
    int alloc() {
        HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&host), lay.total_elems() * sizeof(int32_t), hipHostMallocDefault));
        for (hipEvent_t &e : ev) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        return dev.alloc(lay.total_elems() * sizeof(int32_t));
    }
    // -- the workers' side: where member m's draw of iteration `at` of chunk c goes
    int32_t *host_slot(int m, int c, int at) { return host + lay.index_at(m, c, at); }
    int *host_counts(int m, int c, int at) { return &cnt[lay.count_at(m, c, at)]; }
    // -- the device side (indices(0, 0, 0): the region's first byte)
    const int32_t *indices(int m, int c, int at) const { return dev.as<int32_t>() + lay.index_at(m, c, at); }
    void counts(int c, int at, int *out) const { for (int m = 0; m < lay.members; m++) out[m] = dcnt[lay.count_at(m, c, at)]; }
    Iteration iteration(RingPos p) const {
        Iteration it;
        it.idx0 = indices(0, p.chunk, p.at);
        counts(p.chunk, p.at, it.counts);
        for (int m = 1; m < lay.members; m++) it.same = it.same && it.counts[m] == it.counts[0];
        return it;
    }
    // Chunk c's draws go to the device ring: one copy per member, one event behind them.  The batch sizes are copied out of the
    // host ring at once (the host slot is the samplers' again before the chunk's steps run); the indices stay in the pinned slot
    // until the copy has run.
    int upload(int c) {
        const int len = win.sched.length(c);
        for (int m = 0; m < lay.members; m++) {
            const size_t i0 = lay.index_at(m, c, 0), i1 = lay.index_at(m, c, len), c0 = lay.count_at(m, c, 0), c1 = lay.count_at(m, c, len);
            std::copy(cnt.begin() + c0, cnt.begin() + c1, dcnt.begin() + c0);
            HIP_TRY(hipMemcpyAsync(dev.as<int32_t>() + i0, host + i0, (i1 - i0) * sizeof(int32_t), hipMemcpyHostToDevice, stream));
        }
        HIP_TRY(hipEventRecord(ev[lay.slot(c)], stream));
        win.uploaded_chunk(c);
        return GNN_OK;
    }
    // hands finished uploads' host slots back to the samplers: those whose event has completed -- waiting for the OLDEST one when `wait`
    // (an upload sits in front of the steps of the chunk BEFORE its own, so by the time the samplers need the slot,
    //  kIndexRingSlots chunks later, the copy ran long ago: the wait does not stall)
    int release(bool wait) {
        hipError_t q = hipSuccess; // (the last answer: the error, when the window reports one)
        const bool ok = win.release(wait, [&](int c, bool block) {
            q = block ? hipEventSynchronize(ev[lay.slot(c)]) : hipEventQuery(ev[lay.slot(c)]);
            return q == hipSuccess ? UploadPoll::done : q == hipErrorNotReady ? UploadPoll::not_ready : UploadPoll::error;
        }, [&](int upto) { sr.release(upto); });
        return ok ? GNN_OK : fail(GNN_ERR_HIP, std::string("upload event: ") + hipGetErrorString(q));
    }
    // Chunk c on the device, waiting for its draws if need be -- and chunk c + 1 IN FRONT OF chunk c's steps when the samplers
    // have it (which they have: they run kIndexRingSlots chunks ahead; no waiting for it): the last step of a chunk then knows its
    // successor like every other step, and the chain of two-launch steps runs through the chunk boundary -- an upload in stream
    // order at the boundary left the GPU idle for the copy and restarted the chain with a forward-only launch, ~1 us per step
    // over a run.
    int stage(int c) {
        TRY(release(false));
        if (win.next(c)) {
            // (the samplers may be waiting for a host slot whose upload is still in flight: hand slots back while waiting for them)
            while (!sr.ready(c)) {
                TRY(release(win.full()));
                if (sr.wait_ready(c, 200)) break;
            }
            std::string msg;
            if (const int src = sr.error(&msg)) return fail(src, msg);
            TRY(upload(c));
        }
        if (c + 1 < sr.chunks() && sr.ready(c + 1) && sr.error() == GNN_OK) TRY(upload(c + 1));
        return GNN_OK;
    }
};
} // namespace

// The loop NNT:60-92 on a resident dataset, for n samplers (lone callers: one).
// `obs` (handle.h: SampledObserver) is called behind every step and behind every sampler chunk, on the calling thread, with the
// handle's stream holding everything enqueued so far: the observed loops below and the group's (group.hip) are this loop + one.
// n > 1: `each`, a group call with one sampler per member on member 0's handle.  Sampler m draws batches of batches[m] into
// ring m, and an iteration whose n batch sizes differ is handed to each->mixed_step instead of being stepped here -- unless
// each->sized(): the grouped launches then take every member's own size (each->step_sizes) and every iteration is stepped here.
// Unless sized, the n nominal sizes are equal.  `stepper` (lone handles): it steps every iteration in place of step_on_device_indices.
int gnn::host::train_sampled_run(gnn_mlp *h, gnn_sampler_t *const *samplers, int n, int iterations, const int *batches, double step,
                                 double momentum, int noise, SampledObserver *obs, SampledEach *each, SampledStep *stepper) {
    TRY(check_handle(h));
    if (n < 1 || n > GROUP_MAX || (n > 1 && !each) || (stepper && each)) return fail(GNN_ERR_BAD_ARG, "bad sampler count");
    const bool sized = each && each->sized();
    int batch = batches[0]; // the largest nominal size: the slot stride of every ring, so that member k's index pointer stays member 0's + k * idx_S
    for (int m = 0; m < n; m++) {
        if (!sized && batches[m] != batches[0]) return fail(GNN_ERR_BAD_ARG, "one batch size for all samplers");
        TRY(train_sampled_checks(h, samplers[m], iterations, batches[m], step, noise));
        batch = std::max(batch, batches[m]);
    }
    if (iterations >= 64) try_specialize(h);
    // The exact epoch sampler is serial host work (~10 us per batch of 128: two Fenwick walks per
    // draw) of the same order as a step on the GPU, so it runs AHEAD on a worker thread, chunk by
    // chunk, while this thread uploads finished chunks and enqueues their steps.  The first chunks are short
    // (16, 32, 64, 128, then 256 iterations): nothing runs on the GPU until the first one is sampled, and a 256-batch
    // first chunk kept it idle for 2.5 ms (0.85 us per step of a 3 000-step call).
    // Index storage is a RING of chunk slots on the host and on the device, whatever the run length (NNT:62 runs 500 000
    // iterations): the sampler waits for a free host slot; a device slot is rewritten by a copy that is enqueued on the handle's
    // stream behind the steps that read it.  With n samplers there are n such rings, drawn by min(n, 8) worker threads
    // (sample_ring.h: a grouped step of 8 nets takes 37 us, eight samplers on one thread 80); the chunks are then shortened so
    // that the n rings together stay within the pinned bound (index_ring.h).
    const IndexRingLayout lay{n, IndexRingLayout::chunk_cap(n, batch), batch};
    const ChunkSchedule sched{iterations, lay.cap};
    SampleRing sr(n, lay.slots, sched.chunks());
    DeviceIndexRing ring(lay, sched, h->stream, sr);
    TRY(ring.alloc());
    // (declared behind everything the workers write: they are joined first on every exit path)
    SampleWorkers workers(sr, SampleWorkers::threads_for(n), [&](int m, int c, std::string *msg) -> int {
        int rc = GNN_OK;
        for (int at = 0, len = sched.length(c); at < len && rc == GNN_OK; at++)
            rc = gnn_sampler_sample(samplers[m], batches[m], ring.host_slot(m, c, at), ring.host_counts(m, c, at));
        if (rc != GNN_OK) *msg = gnn_mlp_last_error();
        return rc;
    });
    if (each) each->region(ring.indices(0, 0, 0), lay.slice_elems() * sizeof(int32_t));
    int rc = GNN_OK;
    for (int c = 0; c < sr.chunks() && rc == GNN_OK; c++) {
        rc = ring.stage(c);
        const int i0 = sched.begin(c), len = sched.length(c);
        for (int at = 0; at < len && rc == GNN_OK; at++) {
            const DeviceIndexRing::Iteration it = ring.iteration(RingPos{c, at});
            const RingPos next = h->chain && !stepper ? ring.win.successor(c, at) : RingPos{};
            const DeviceIndexRing::Iteration nx = next ? ring.iteration(next) : DeviceIndexRing::Iteration{}; // the one to announce, if it is on the device already
            if (stepper) { // (handle.h: SampledStep)
                rc = stepper->step(it.idx0, it.counts[0]);
            } else if (!sized && !it.same) { // the members' batches differ in size (a refill shortened some): member after member, nothing announced
                const int32_t *idx[GROUP_MAX];
                for (int m = 0; m < n; m++) idx[m] = ring.indices(m, c, at);
                rc = each->mixed_step(idx, it.counts);
            } else {
                // (sized: every member with its own size, in the two grouped launches -- the sizes travel beside the announcement)
                if (sized) each->step_sizes(it.counts, nx ? nx.counts : nullptr);
                if (nx && (sized || nx.same)) h->la.announce(NextBatch{h->DX, nx.idx0, nx.counts[0]});
                rc = step_on_device_indices(h, it.idx0, it.counts[0], step, momentum);
            }
            // (a validation pass reads the weights the step has just written; it touches neither the slabs the step's tile
            //  kernel made for the next batch nor the staged rows, so the chain of two-launch steps runs on behind it)
            if (rc == GNN_OK && obs) rc = obs->after_step(i0 + at);
        }
        if (rc == GNN_OK && obs) rc = obs->after_chunk(i0 + len);
    }
    // (on an early exit the sampler stops after the chunk it is drawing: its state stays well defined)
    (void)hipStreamSynchronize(h->stream); // the device ring is released below
    h->la.rows_renamed(); // (they may name rows through the device ring)
    if (each) each->region(nullptr, 0);
    return rc;
}

// ---- the held-out curve and the best weights (keep_best_kernel.h) --------------------------------------------------------------
// A handle's snapshot buffer and its history of the running best: ordinary allocations made at the first call, kept for later
// calls, freed with the handle.
int gnn::host::ensure_keep_best(gnn_mlp *h, int points) {
    if (!h->best_W) {
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&h->best_W), sizeof(float) * (size_t)h->n_pad));
        HIP_TRY(hipMemsetAsync(h->best_W, 0, sizeof(float) * (size_t)h->n_pad, h->stream));
    }
    if (h->best_hist_cap < points) {
        HIP_TRY(hipStreamSynchronize(h->stream)); // (nothing queued may still write the shorter history)
        if (h->best_hist) (void)hipFree(h->best_hist);
        h->best_hist = nullptr; h->best_hist_cap = 0;
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&h->best_hist), sizeof(KeepBestRecord) * (size_t)points));
        h->best_hist_cap = points;
    }
    return GNN_OK;
}
// One launch for the K nets of m (one shape): point `point`'s results hits[k] / loss[k] against record point - 1 of each history
int gnn::host::launch_keep_best(hipStream_t stream, gnn_mlp *const *m, int K, const unsigned long long *hits, const double *loss, int point, int rule) {
    KeepBestParams kp{};
    for (int k = 0; k < K; k++) { kp.W[k] = m[k]->W; kp.snap[k] = m[k]->best_W; kp.hist[k] = m[k]->best_hist; }
    kp.hits = hits; kp.loss = loss;
    kp.n4 = (unsigned)(m[0]->n_pad / 4);
    kp.point = point; kp.rule = rule;
    const unsigned per_block = KB_NT * KB_VEC;
    hipLaunchKernelGGL(keep_best_kernel, dim3((kp.n4 + per_block - 1) / per_block, (unsigned)K), dim3(KB_NT), 0, stream, kp);
    HIP_TRY(hipGetLastError());
    return GNN_OK;
}
int gnn::host::check_held_out_args(const gnn_mlp *h, int every, int64_t held_rows, int rule, const void *point_hits, const void *point_loss,
                                   const void *best_point) {
    if (!point_hits || !point_loss || !best_point) return fail(GNN_ERR_BAD_ARG, "null output");
    if (rule != GNN_BEST_LOSS && rule != GNN_BEST_HITS) return fail(GNN_ERR_BAD_ARG, "rule: GNN_BEST_LOSS or GNN_BEST_HITS");
    if (every < 1) return fail(GNN_ERR_BAD_ARG, "every must be positive");
    if (!h->held.X) return fail(GNN_ERR_STATE, "no held-out set uploaded");
    if (held_rows < 1 || held_rows > h->held.n) return fail(GNN_ERR_BAD_ARG, "held_rows outside the held-out set");
    return GNN_OK;
}

namespace {
// Behind the iterations that end an interval: the pass of gnn_mlp_evaluate_set_range over the held-out rows with its results
// left in slot p of d_res ([P][hits, loss sum]), then the keep_best launch.  Behind the last chunk, in front of the loop's own
// wait for the stream: the readbacks.
struct LoneHeldOut : SampledObserver {
    gnn_mlp *h; int iterations, every, rule, P; int64_t held_rows;
    unsigned long long *d_res;
    bool want_weights;
    std::vector<unsigned long long> res; KeepBestRecord best{0, 0.0, -1, 0}; std::vector<float> w;
    int after_step(int i) override {
        if ((i + 1) % every != 0 && i + 1 != iterations) return GNN_OK;
        const int p = i / every;
        unsigned long long *hits = d_res + 2 * (size_t)p;
        double *loss = reinterpret_cast<double *>(hits + 1);
        TRY(enqueue_evaluation(h, h->held, 0, held_rows, hits, loss, nullptr, nullptr));
        return launch_keep_best(h->stream, &h, 1, hits, loss, p, rule);
    }
    int after_chunk(int i_end) override {
        TRY_LAUNCHES(h);
        if (i_end != iterations) return GNN_OK;
        HIP_TRY(hipMemcpyAsync(res.data(), d_res, sizeof(unsigned long long) * res.size(), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(&best, h->best_hist + (P - 1), sizeof(KeepBestRecord), hipMemcpyDeviceToHost, h->stream));
        if (want_weights) HIP_TRY(hipMemcpyAsync(w.data(), h->best_W, sizeof(float) * w.size(), hipMemcpyDeviceToHost, h->stream));
        return GNN_OK;
    }
};
} // namespace

extern "C" {

int gnn_mlp_held_out_points(int iterations, int every) {
    if (iterations < 1 || every < 1) return -1;
    return (int)(((int64_t)iterations + every - 1) / every);
}

int gnn_mlp_train_sampled_held_out(gnn_mlp_t *h, gnn_sampler_t *s, int iterations, int batch, double step, double momentum,
                                   int noise, int every, int64_t held_rows, int rule, int64_t *point_hits, double *point_loss,
                                   int32_t *best_point, double *best_weights) { return guarded([&]() -> int {
    TRY(check_handle(h));
    TRY(train_sampled_checks(h, s, iterations, batch, step, noise));
    TRY(check_held_out_args(h, every, held_rows, rule, point_hits, point_loss, best_point));
    const int P = gnn_mlp_held_out_points(iterations, every);
    TRY(ensure_keep_best(h, P));
    { // (the evaluation workspace a point may need, grown before the first step)
        int rc_ws = GNN_OK;
        EvalScope scope(h, eval_block_rows(h, held_rows), &rc_ws);
        if (rc_ws != GNN_OK) return rc_ws;
    }
    DevScratch dres;
    TRY(dres.alloc(sizeof(unsigned long long) * 2 * (size_t)P));
    HIP_TRY(hipMemsetAsync(dres.p, 0, sizeof(unsigned long long) * 2 * (size_t)P, h->stream));
    LoneHeldOut obs;
    obs.h = h; obs.iterations = iterations; obs.every = every; obs.rule = rule; obs.P = P; obs.held_rows = held_rows;
    obs.d_res = dres.as<unsigned long long>();
    obs.want_weights = best_weights != nullptr;
    obs.res.assign(2 * (size_t)P, 0);
    if (best_weights) obs.w.assign((size_t)h->n_pad, 0.f);
    TRY(train_sampled_run(h, &s, 1, iterations, &batch, step, momentum, noise, &obs, nullptr));
    // (the loop has waited for the stream behind the readbacks: the ONE synchronisation)
    static_assert(sizeof(unsigned long long) == sizeof(double), "one buffer for counters and sums");
    for (int p = 0; p < P; p++) {
        point_hits[p] = (int64_t)obs.res[2 * (size_t)p];
        std::memcpy(&point_loss[p], &obs.res[2 * (size_t)p + 1], sizeof(double));
    }
    *best_point = obs.best.at;
    if (best_weights && obs.best.at >= 0) unpack_params(h, obs.w, best_weights);
    return GNN_OK;
}); }

} // extern "C"

namespace {
// The observed variants (NNT:68-72, 75-79) of a lone handle: after iteration i the summed validation loss of rows
// [0, validation_size) goes to d_val[i] (device).
struct LoneValidation : SampledObserver {
    gnn_mlp *h; int validation_size; double *d_val; float *d_rows; int64_t row_stride;
    LoneValidation(gnn_mlp *h_, int n, double *dv, float *dr, int64_t rs) : h(h_), validation_size(n), d_val(dv), d_rows(dr), row_stride(rs) {}
    int after_step(int i) override {
        // the per-sample losses of iteration i stay in row i of d_rows (summed once, behind the loop); a validation set of
        // more than one block is summed block by block as before
        int vrc = GNN_OK;
        if (d_rows && validation_losses_to_row(h, validation_size, d_rows + (size_t)i * row_stride, &vrc)) return vrc;
        return validation_loss_sum(h, validation_size, d_val + i);
    }
};
} // namespace

extern "C" {

int gnn_mlp_train_sampled(gnn_mlp_t *h, gnn_sampler_t *s, int iterations, int batch, double step, double momentum,
                          int noise) { return guarded([&]() -> int {
    return train_sampled_run(h, &s, 1, iterations, &batch, step, momentum, noise, nullptr, nullptr);
}); }

int gnn_mlp_train_sampled_observed(gnn_mlp_t *h, gnn_sampler_t *s, int iterations, int batch, double step, double momentum,
                                   int noise, int validation_size, double *val_loss) { return guarded([&]() -> int {
    TRY(check_handle(h));
    if (!val_loss) return fail(GNN_ERR_BAD_ARG, "null output");
    if (iterations <= 0) return fail(GNN_ERR_BAD_ARG, "iterations must be positive (NNT:62)");
    if (validation_size <= 0 || validation_size > h->dataset_n) return fail(GNN_ERR_BAD_ARG, "validation size outside the dataset (NNT:104)");
    DevScratch dv, drows;
    TRY(dv.alloc(sizeof(double) * (size_t)iterations));
    // one row of per-sample losses per iteration when the validation set is ONE forward block (601 rows at MNIST's size): the rows
    // are summed by one launch behind the loop instead of one per iteration.  (Capped at 1 GiB: longer calls sum per iteration.)
    const int64_t stride = pad_up(validation_size);
    const bool rows_form = eval_block_rows(h, validation_size) >= validation_size && (int64_t)iterations * stride * 4 <= (1ll << 30);
    if (rows_form) TRY(drows.alloc(sizeof(float) * (size_t)iterations * (size_t)stride));
    LoneValidation obs(h, validation_size, dv.as<double>(), rows_form ? drows.as<float>() : nullptr, stride);
    TRY(train_sampled_run(h, &s, 1, iterations, &batch, step, momentum, noise, &obs, nullptr));
    if (rows_form) {
        hipLaunchKernelGGL(sum_rows_kernel, dim3(iterations), dim3(256), 0, h->stream, RowSumParams{drows.as<float>(), stride, validation_size, dv.as<double>()});
        TRY_LAUNCHES(h);
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    // (train_sampled_run has waited for the stream: every sum is in place)
    HIP_TRY(hipMemcpy(val_loss, dv.p, sizeof(double) * (size_t)iterations, hipMemcpyDeviceToHost));
    for (int i = 0; i < iterations; i++) val_loss[i] /= (double)validation_size; // NNT:112
    return GNN_OK;
}); }

} // extern "C"
