/*
 * gnn_mlp.h -- C ABI of the MI355X-native (gfx950) MLP mini-batch SGD path.
 *
 * This is the drop-in boundary for the hot path of asheptunov/graph-neural-net: the
 * arithmetic of SoftmaxCrossEntropyNeuralNet / GeneralNeuralNet (the two implementations of
 * the `NeuralNet` operator interface) moves behind these entry points; the Java NeuralNet /
 * NeuralNetTrainer API surface above it stays.  The reference has no FFI of its own; the
 * functions below are what a JNI shim for its `NeuralNet` interface binds (INTEGRATION.md shows
 * the Java `native` declarations and the JNI stub for each).
 *
 * Citations are file:line under /root/reference/src.  NN = NeuralNet.java,
 * SCE = SoftmaxCrossEntropyNeuralNet.java, GNN = GeneralNeuralNet.java,
 * NNT = NeuralNetTrainer.java, MT = MNISTTrainer.java.
 *
 * Conventions
 *  - plain C types only; every function returns a gnn_status (0 = ok) and never throws or
 *    aborts across the ABI; gnn_mlp_last_error() gives the message of the calling thread's
 *    last failure.
 *  - host matrices are dense row-major fp64, exactly the reference's `double[]` rows laid end
 *    to end: X is B x d_0, Y is B x d_{L-1}.  The reference passes one sample (or a
 *    Map<double[],double[]>) per call; the shim flattens the Map in iteration order.
 *  - flat parameter vectors (weights, momentum, gradients) are layer-major, each layer
 *    row-major [in][out] like `weights.get(l)[in][out]` (SCE:44-47), UNPADDED, fp64 on the host.
 *  - the library never keeps a host pointer past the call (the reference aliases the caller's
 *    input array in neurons[0], SCE:167-168; no caller can observe that through NN:16-65).
 *  - one gnn_mlp_t = one GPU = one logical stream of calls (gnn_mlp_dp_t: one handle over N GPUs); calls on one handle must be serialised
 *    by the caller (the reference classes are not re-entrant either: `neurons` is shared scratch).
 *  - there is NO CPU fallback: with no gfx950 device every entry point fails with
 *    GNN_ERR_NO_DEVICE.
 */
#ifndef GNN_MLP_H
#define GNN_MLP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: only what this header declares is exported */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

typedef struct gnn_mlp gnn_mlp_t;

typedef enum {
    GNN_OK = 0,
    GNN_ERR_BAD_ARG = 1,     /* null pointer, bad dims, B out of range ... (reference: `assert`) */
    GNN_ERR_HIP = 2,         /* a HIP runtime call failed; message holds hipGetErrorString */
    GNN_ERR_UNSUPPORTED = 3, /* e.g. noise=1 (SCE:334-336 is NaN-producing) */
    GNN_ERR_NO_DEVICE = 4,   /* no HIP device visible */
    GNN_ERR_STATE = 5        /* e.g. indexed step before a dataset was uploaded */
} gnn_status;

/* Closed enum standing in for the reference's ActivationFunction / ActivationPrime lambdas
 * (ActivationFunction.java:14, ActivationPrime.java:14).  LEAKY_RELU is the pair the
 * reference ships: a>0 ? a : 0.01a  and  a<=0 ? 0.01 : 1.0  (MT:234-235). */
typedef enum {
    GNN_ACT_LEAKY_RELU = 0,
    GNN_ACT_SIGMOID = 1,
    GNN_ACT_TANH = 2,
    GNN_ACT_RELU = 3,
    GNN_ACT_IDENTITY = 4
} gnn_act;

typedef enum {
    GNN_OUT_SOFTMAX_CE = 0, /* SoftmaxCrossEntropyNeuralNet: softmax + cross entropy (SCE:197,216,250) */
    GNN_OUT_ACT_LOSS = 1    /* GeneralNeuralNet: last_act + loss (GNN:215-218,238,267-271) */
} gnn_out_kind;

typedef enum {
    GNN_LOSS_HALF_SQUARED = 0 /* 0.5*(a-y)^2, derivative (a-y)  (LossFunction.java:16) */
} gnn_loss;

typedef enum {
    GNN_DTYPE_F32 = 0, /* f32 operands, f32 MFMA (v_mfma_f32_16x16x4_f32), f32 accumulate */
    GNN_DTYPE_BF16 = 1 /* bf16 GEMM operands, f32 accumulate, f32 master weights + momentum */
} gnn_dtype;

/* ---- construction (SCE:103-128 / GNN:112-147) ------------------------------------------- */

/* Builds the net on HIP device `device` and draws the initial weights exactly as
 * appendLayer does (SCE:139-156): java.util.Random(seed), layer by layer, row-major,
 * nextDouble() - 0.5; momentum ("previousUpdate") zero; time 0.  The reference hard-codes
 * seed 1 (SCE:111).  `last_act`/`loss` are ignored for GNN_OUT_SOFTMAX_CE.
 * `max_batch` bounds B of every later call (device buffers are sized once, here). */
int gnn_mlp_create(const int32_t *dims, int n_dims, int out_kind, int inner_act, int last_act,
                   int loss, int64_t seed, int dtype, int device, int max_batch,
                   gnn_mlp_t **out);
int gnn_mlp_destroy(gnn_mlp_t *h);

int gnn_mlp_input_dim(const gnn_mlp_t *h);    /* NN:58 getInputDim  (SCE:383) */
int gnn_mlp_output_dim(const gnn_mlp_t *h);   /* NN:65 getOutputDim (SCE:392) */
int64_t gnn_mlp_num_params(const gnn_mlp_t *h); /* sum_l d_l*d_{l+1} */
int gnn_mlp_time(const gnn_mlp_t *h);         /* `time`: gradient steps taken (SCE:23,343) */
const char *gnn_mlp_last_error(void);

/* ---- the NeuralNet operator interface, batched ------------------------------------------ */

/* NN:16 propagate (SCE:164-198, GNN:183-221) for B samples: out is B x d_{L-1}
 * (softmax probabilities, or last_act(z) for GNN_OUT_ACT_LOSS).  Synchronous. */
int gnn_mlp_propagate(gnn_mlp_t *h, const double *X, int B, double *out);

/* NN:27 calculateLoss (SCE:207-220, GNN:230-242): loss_per_sample has B entries. */
int gnn_mlp_loss(gnn_mlp_t *h, const double *X, const double *Y, int B, double *loss_per_sample);

/* NN:39 calculateWeightGradient (SCE:229-287, GNN:251-307), summed over the B samples
 * (B = 1 reproduces the reference call); flat_grad has gnn_mlp_num_params entries. */
int gnn_mlp_weight_gradient(gnn_mlp_t *h, const double *X, const double *Y, int B,
                            double *flat_grad);

/* NN:51 gradientStep (SCE:297-346, GNN:317-366): G = sum over the batch of the per-sample
 * gradients; adj = step*G/B + momentum*prev; W -= adj; prev = adj; time++.
 * noise != 0 -> GNN_ERR_UNSUPPORTED.  Returns after enqueueing (asynchronous).  On the small-net path the weight UPDATE of a
 * call is enqueued with the NEXT gradient_step call (one kernel then applies it and starts the new batch: three dependent
 * launches per call instead of four), or by whichever other entry point of the handle is called first -- every entry point
 * sees the updated weights, `time` counts the step at the call, results are the same bit for bit (GNN_MLP_DEFER=0 switches
 * it off). */
int gnn_mlp_gradient_step(gnn_mlp_t *h, const double *X, const double *Y, int B, double step,
                          double momentum, int noise);

/* MT:166-168 / MT:191-193 argmax of propagate(): `>=`, so ties go to the HIGHEST index. */
int gnn_mlp_argmax(gnn_mlp_t *h, const double *X, int B, int32_t *labels);

/* ---- parameter access (extension: `weights` is private with no getter, SCE:15) ----------- */
int gnn_mlp_get_weights(gnn_mlp_t *h, double *flat);
int gnn_mlp_set_weights(gnn_mlp_t *h, const double *flat);
int gnn_mlp_get_momentum(gnn_mlp_t *h, double *flat);
int gnn_mlp_set_momentum(gnn_mlp_t *h, const double *flat);

/* Checkpoint (the reference has no persistence at all: a trained net is lost at JVM exit,
 * SURVEY 5).  File, little endian: "GNNMLP2\0", int32 L, int32 dims[L], int32 out_kind, inner_act,
 * last_act, loss, dtype, int32 time, int64 P, fp64 weights[P], fp64 momentum[P] (flat layer-major
 * row-major [in][out] like get_weights), uint64 FNV-1a of all preceding bytes.  Loading requires
 * identical dims AND configuration (a sigmoid / bf16 / GeneralNeuralNet file is refused by a
 * leaky-ReLU / f32 / softmax net of the same dims) and an intact payload (length and checksum). */
int gnn_mlp_save_checkpoint(gnn_mlp_t *h, const char *path);
int gnn_mlp_load_checkpoint(gnn_mlp_t *h, const char *path);

/* ---- device-resident training data (the caller of the path: NNT:28-43, NNT:143-168) ------ */

/* Copies N samples to HBM once (fp64 -> compute dtype, inner activation applied to the input
 * as SCE:183-186 does for layer 0).  Later *_indexed / *_range calls do no host->device copy
 * of sample data. */
int gnn_mlp_upload_dataset(gnn_mlp_t *h, const double *X, const double *Y, int64_t N);
/* Same from raw IDX payloads with the reference's encoding done on the GPU:
 * pixel -> (byte & 0xff)/255.0 (MT:98), label -> one-hot 1.0 (MT:112-118). */
int gnn_mlp_upload_dataset_u8(gnn_mlp_t *h, const uint8_t *pixels, const uint8_t *labels,
                              int64_t N);
int64_t gnn_mlp_dataset_size(const gnn_mlp_t *h);

/* gradientStep on dataset rows idx[0..B) (host int32 indices, e.g. one NNT.sample draw). */
int gnn_mlp_gradient_step_indexed(gnn_mlp_t *h, const int32_t *idx, int B, double step,
                                  double momentum, int noise);
/* gradientStep on the contiguous dataset rows [first, first+B). */
int gnn_mlp_gradient_step_range(gnn_mlp_t *h, int64_t first, int B, double step,
                                double momentum, int noise);
/* n_steps consecutive gradientSteps (the loop NNT:82-85) over rows
 * [first + s*B, first + (s+1)*B) mod the rows that fit, s = 0..n_steps-1, with no host work
 * between steps. */
int gnn_mlp_train_range(gnn_mlp_t *h, int64_t first, int B, int n_steps, double step,
                        double momentum);
int gnn_mlp_loss_range(gnn_mlp_t *h, int64_t first, int B, double *loss_per_sample);
int gnn_mlp_argmax_range(gnn_mlp_t *h, int64_t first, int B, int32_t *labels);
/* testOnTrainingData / testOnTestData (MT:159-197) over the dataset rows [first, first + n), any n: propagate + the `>=`
 * argmax (MT:166-168) per row, a hit when it equals the expected class -- the LAST index whose expected value is 1
 * (MT:186-188; for the one-hot rows of MT:112-118 that is the label).  The rows are walked in blocks of max_batch with no host
 * work in between; ONE count comes back.  The reference returns hits / size (MT:172, 197): the division is the caller's. */
int gnn_mlp_count_hits_range(gnn_mlp_t *h, int64_t first, int64_t n, int64_t *hits);
/* The same pass (MT:159-197) with everything it has on the device returned from ONE readback, any n: *hits as
 * gnn_mlp_count_hits_range counts them; *loss_sum = the sum of calculateLoss over the rows (validate() of NNT:102-113 without its
 * division), added block after block in one fixed order; confusion[e * d_out + p] = the number of rows whose expected class
 * (MT:186-188) is e and whose `>=` argmax (MT:166-168) is p -- row = expected, column = predicted, the trace is *hits --;
 * labels[i] = the argmax of row first + i.  Each of the four may be null, not all of them.  Works on borrowed handles (group
 * members, data-parallel replicas); bf16 handles walk blocks of max_batch rows. */
int gnn_mlp_evaluate_range(gnn_mlp_t *h, int64_t first, int64_t n, int64_t *hits, double *loss_sum,
                           int64_t *confusion /* [d_out][d_out] */, int32_t *labels /* [n] */);

/* Which inputs the loss depends on: grad[b * d_0 + i] = d calculateLoss(X_b, Y_b) / d X_b[i] (NN:27, SCE:207-220, GNN:230-242)
 * -- the l = 0 continuation of the backward loop the reference stops at delta_1 (SCE:272-278):
 * (delta_1 . W_0^T) * f'(x), f' because the reference applies f to the raw input too (SCE:183-186); f' is taken from f(x), for
 * the leaky pair `<= 0 ? 0.01 : 1` (MT:235), so an exact-zero input gets 0.01.  With two layers delta_1 is the output delta.
 * bf16 handles take delta_1 and W_0 rounded to bf16 with f32 accumulation.  Host rows, 1 <= B <= max_batch.  The handle's
 * own gradient computation runs first: like gnn_mlp_compute_gradient* the call leaves the gradient buffer holding (its last
 * block's) weight gradient; it changes no weight, momentum, step count or sampler, and a deferred host-batch update is applied
 * first.  Works on borrowed handles and on every plan (csrc/input_grad_kernel.h: one more launch per block of rows). */
int gnn_mlp_input_gradient(gnn_mlp_t *h, const double *X, const double *Y, int B, double *grad /* [B][d_0] */);
/* The same over the dataset rows [first, first + n), any n, in blocks of max_batch with no host work in between and ONE
 * readback: grad as above; saliency[e * d_0 + i] = the sum of |grad[.][i]| over the rows whose expected class (MT:186-188) is e,
 * added in fp64 in row order (the same bits every time); class_rows[e] = the number of those rows.  Each of the three may be
 * null, not all of them. */
int gnn_mlp_input_gradient_range(gnn_mlp_t *h, int64_t first, int64_t n, double *grad /* [n][d_0] or null */,
                                 double *saliency /* [d_out][d_0] or null */, int64_t *class_rows /* [d_out] or null */);

/* ---- the trainer's sampling loop (NeuralNetTrainer.java) ------------------------------------ */

/* Epoch sampler without replacement, NNT:28-43 + NNT:143-168: java.util.Random(seed) (the
 * reference uses 1, NNT:42), nextInt(remaining) picks the r-th REMAINING sample in master order
 * (ArrayList.get(r) + remove(r), NNT:152-154), the list refills when empty -- also in the middle
 * of a batch (NNT:149-151), in which case a sample drawn twice collapses in the reference's
 * HashMap (NNT:155) and the batch is shorter than requested.  Master order here is
 * dataset row order (the reference's is HashMap iteration order, i.e. unspecified). */
typedef struct gnn_sampler gnn_sampler_t;
int gnn_sampler_create(int32_t master_size, int64_t seed, gnn_sampler_t **out);
int gnn_sampler_destroy(gnn_sampler_t *s);
/* One sample(batchSize) call: writes the DISTINCT rows in first-draw order, *n_out of them. */
int gnn_sampler_sample(gnn_sampler_t *s, int batch, int32_t *out_idx, int *n_out);
/* The loop NNT:82-85 / NNT:88-90: `iterations` times { sample(batch); gradientStep }. All draws
 * are made up front and uploaded once; the steps are then enqueued with no host->device copy. */
int gnn_mlp_train_sampled(gnn_mlp_t *h, gnn_sampler_t *s, int iterations, int batch, double step,
                          double momentum, int noise);
/* The OBSERVED loops NNT:68-72 / NNT:75-79: `iterations` times { sample(batch); gradientStep; validate(validation_size) }.
 * validate (NNT:102-113) is the mean of calculateLoss over the first validation_size samples in master order -- here dataset
 * rows [0, validation_size).  Steps and validation passes are enqueued back to back; the summed losses stay in a device buffer
 * and come back ONCE: val_loss[i] = validate(validation_size) after iteration i (the value the reference prints as "%d,%.2f",
 * NNT:71).  Needs 0 < validation_size <= the dataset's size. */
int gnn_mlp_train_sampled_observed(gnn_mlp_t *h, gnn_sampler_t *s, int iterations, int batch, double step,
                                   double momentum, int noise, int validation_size, double *val_loss);

/* ---- the held-out set (MNISTTrainer's test rows, MT:98, MT:159-172) ------------------------------
 * A second resident data set beside the training set: the same layout and encodings (gnn_mlp_upload_dataset / _u8), read by
 * the evaluation passes only.  An upload replaces the previous held-out set after a stream synchronisation; it touches neither
 * the training set nor the look-ahead state (no training row is renamed) nor a pending host-batch update's result, and
 * uploading the training set leaves the held-out set alone.  On a member of a group -> GNN_ERR_STATE (the group holds ONE
 * copy: gnn_mlp_group_upload_held_out).  Freed with its owner. */
typedef enum { GNN_SET_TRAIN = 0, GNN_SET_HELD_OUT = 1 } gnn_data_set;
int gnn_mlp_upload_held_out(gnn_mlp_t *h, const double *X, const double *Y, int64_t N);
int gnn_mlp_upload_held_out_u8(gnn_mlp_t *h, const uint8_t *pixels, const uint8_t *labels, int64_t N);
/* rows of the named set: 0 when nothing was uploaded, -1 for a null handle or a `set` that is neither value */
int64_t gnn_mlp_set_rows(const gnn_mlp_t *h, int set);
/* gnn_mlp_evaluate_range with the set named: testOnTrainingData (MT:180-197) with GNN_SET_TRAIN -- bit for bit
 * gnn_mlp_evaluate_range --, testOnTestData (MT:159-172) with GNN_SET_HELD_OUT -- bit for bit what gnn_mlp_evaluate_range
 * returns on a handle with the same weights whose training set is those rows.  The same launches, block sizes and summing
 * order; one readback; writes no weight, momentum, step count or look-ahead state.  The named set never uploaded ->
 * GNN_ERR_STATE; rows outside it, or a `set` that is neither value -> GNN_ERR_BAD_ARG.  The two accuracies are one row of
 * logs/trainLog.csv (MT:241). */
int gnn_mlp_evaluate_set_range(gnn_mlp_t *h, int set, int64_t first, int64_t n, int64_t *hits, double *loss_sum,
                               int64_t *confusion /* [d_out][d_out] */, int32_t *labels /* [n] */);

/* A training loop with a held-out curve that keeps the best weights ON THE DEVICE (csrc/keep_best_kernel.h).  Trains exactly
 * as gnn_mlp_train_sampled: weights, momentum, `time` and the sampler end bit for bit where that call leaves them.  Point p in
 * [0, P), P = gnn_mlp_held_out_points(iterations, every) = ceil(iterations / every), is taken after iteration
 * min((p + 1) * every, iterations), counted from 1: rows [0, held_rows) of the held-out set are evaluated on the device,
 * point_hits[p] and point_loss[p] (the SUM, like loss_sum) bit for bit what gnn_mlp_evaluate_set_range(h, GNN_SET_HELD_OUT, 0,
 * held_rows, ..) would return at that moment (testOnTestData, MT:159-172, along the run).  The running best is decided in point
 * order, starting from "none".  Point p becomes the best when
 *   GNN_BEST_LOSS: its loss is not NaN and (there is no best yet, or its loss is strictly lower);
 *   GNN_BEST_HITS: there is no best yet, or it has strictly more hits, or equal hits and a strictly lower loss (a NaN loss is
 *                  never lower).
 * Ties keep the earlier point.  *best_point = the final best, -1 when GNN_BEST_LOSS never saw a number.  best_weights, when not
 * null, receives the weights the net held AT that point, in the layout of gnn_mlp_get_weights and bit for bit what that call
 * would have returned there; left unwritten when *best_point is -1.  A point is one launch behind its evaluation launches and
 * writes nothing the step reads: the chain of two-launch steps runs on behind it; curves, *best_point and the weights come back
 * behind ONE synchronisation.  Refused before any step and any draw: every < 1, held_rows outside [1, held-out rows], a null
 * point_hits / point_loss / best_point, a `rule` that is neither value -> GNN_ERR_BAD_ARG; no held-out set -> GNN_ERR_STATE;
 * noise != 0 -> GNN_ERR_UNSUPPORTED; everything gnn_mlp_train_sampled refuses, with its codes. */
typedef enum { GNN_BEST_LOSS = 0, GNN_BEST_HITS = 1 } gnn_best_rule;
int gnn_mlp_held_out_points(int iterations, int every); /* P; -1 unless iterations >= 1 and every >= 1 */
int gnn_mlp_train_sampled_held_out(gnn_mlp_t *h, gnn_sampler_t *s, int iterations, int batch, double step, double momentum,
                                   int noise, int every, int64_t held_rows, int rule,
                                   int64_t *point_hits /* [P] */, double *point_loss /* [P] */,
                                   int32_t *best_point, double *best_weights /* [num_params] or null */);

/* ---- data-parallel hooks (one process per GPU; the exchange is the caller's collective) -- */

/* The reference sums per-sample gradients at SCE:305-322 and divides by batch.size() at
 * SCE:333.  Sharded over ranks that sum becomes: each rank's partial G (its rows only) ->
 * all-reduce(SUM) of the flat device gradient buffer -> identical update on every rank with
 * B_global.  The buffer is fp32, gnn_mlp_grad_elems() long (padded layout, pads are zero). */
int64_t gnn_mlp_grad_elems(const gnn_mlp_t *h);
int gnn_mlp_grad_device_ptr(gnn_mlp_t *h, void **dev_ptr);
/* Use a caller-owned device buffer (e.g. a torch tensor registered with RCCL) instead. */
int gnn_mlp_bind_grad_buffer(gnn_mlp_t *h, void *dev_ptr, int64_t n_elems);
/* Run all kernels on the caller's hipStream_t (e.g. torch's current stream); NULL = own. */
int gnn_mlp_set_stream(gnn_mlp_t *h, void *hip_stream);
/* forward + backward of dataset rows [first, first+B_local) into the gradient buffer. */
int gnn_mlp_compute_gradient_range(gnn_mlp_t *h, int64_t first, int B_local);
int gnn_mlp_compute_gradient(gnn_mlp_t *h, const double *X, const double *Y, int B_local);
/* SCE:324-344 on the (all-reduced) gradient buffer with batchSize = B_global. */
int gnn_mlp_apply_update(gnn_mlp_t *h, int B_global, double step, double momentum);
/* Optional: names the dataset rows [first, first+B) that the NEXT gradient computation will run on
 * (the loop NNT:82-85 knows its next batch).  On the small-net path the kernel that updates the
 * weights then also forms that batch's first-layer sums, tile by tile, from the weights it has just
 * written (one dependent launch less per step).  Good for one update; results do not depend on it. */
int gnn_mlp_hint_next_range(gnn_mlp_t *h, int64_t first, int B);
int gnn_mlp_synchronize(gnn_mlp_t *h);
/* A caller that captured steps into a hipGraph (stream capture on the stream given to
 * gnn_mlp_set_stream) replays device work the host-side `time` counter (SCE:343) does not see;
 * it reports the replayed steps here (and takes back, with a negative count, the steps that
 * were only captured, not executed). */
int gnn_mlp_advance_time(gnn_mlp_t *h, int steps);
/* Drops what the handle remembers about work done AHEAD of the next gradient computation (the next batch's first-layer
 * sums made by the previous step's tile kernel, a pending gnn_mlp_hint_next_range).  The next gradient computation then
 * starts its own chain: results are unchanged (bitwise), one extra launch.  A caller that captures
 * gnn_mlp_compute_gradient_range / gnn_mlp_apply_update into a HIP graph itself MUST call this before the capture begins
 * (so that the captured sequence does not depend on what ran before it), after it ends, and after every replay (the host
 * bookkeeping describes the captured pass, not what the device then holds).  gnn_mlp_train_range's own captured pass
 * (GNN_MLP_GRAPH=1) is a closed chain -- it starts and ends on the same batch -- and keeps that bookkeeping consistent itself. */
int gnn_mlp_forget_lookahead(gnn_mlp_t *h);
/* After a stream capture that FAILED (e.g. a collective that cannot be captured invalidated it):
 * ends a capture still open on the handle's stream, discards its graph and clears the sticky HIP
 * error of the calling thread, so that eager calls work again; if the runtime keeps the stream
 * in the invalidated state the handle returns to its own stream and the caller binds a fresh one
 * with gnn_mlp_set_stream. No reference counterpart. */
int gnn_mlp_recover_stream(gnn_mlp_t *h);

/* ---- one process per GPU, the exchange INSIDE the library's step loop -------------------------------------------------
 * The partitioning of the hooks above (rows sharded over the ranks, ONE sum of the flat gradient per step, the identical
 * update with batchSize = B_global, SCE:305-322 / SCE:333) with the sum done by the library itself: every rank process attaches
 * an RCCL communicator to its handle (ncclCommInitRank; RCCL is loaded at run time) and then runs n_steps steps in ONE call --
 * gradient kernels, ncclAllReduce on the same stream, update kernel, no host work of the caller's in between.
 *   rank 0:      gnn_mlp_rccl_unique_id(id)            -> 128 bytes, handed to every rank by the caller (a torch.distributed
 *                                                         store, MPI, a file: the library does no rendezvous of its own)
 *   every rank:  gnn_mlp_rccl_attach(h, id, n_ranks, rank)   (collective: returns when all ranks have joined)
 *                gnn_mlp_rccl_train_range(h, first, B_local, n_steps, step, momentum)   rows [first + s B_local, ..) of THIS
 *                                                         rank's resident data set per step; batchSize = B_local * n_ranks
 * Replicas stay bitwise identical (the all-reduce leaves the same bits on every rank).  UNVERIFIED beyond a world of one rank:
 * the build boxes have one GPU. */
int gnn_mlp_rccl_unique_id(void *id128);
int gnn_mlp_rccl_attach(gnn_mlp_t *h, const void *id128, int n_ranks, int rank);
int gnn_mlp_rccl_detach(gnn_mlp_t *h);
int gnn_mlp_rccl_train_range(gnn_mlp_t *h, int64_t first, int B_local, int n_steps, double step, double momentum);

/* ---- data parallel INSIDE the library: one handle, N device replicas -------------------------------
 * For a caller that is one thread in one process (the reference: NeuralNetTrainer calls gradientStep from
 * the JVM's main thread, NNT:83).  The batch's rows are dealt to the replicas in contiguous blocks, every
 * replica forms the partial gradient of its rows (the per-sample loop SCE:305-322 restricted to them), the
 * flat gradient buffers are summed across the devices, and every replica applies the identical update with
 * batchSize = B (SCE:333): replicas stay bitwise identical.  `max_batch` bounds the GLOBAL batch.
 *   GNN_REDUCE_RCCL   : ncclCommInitAll + one ncclAllReduce(SUM) per replica per step (RCCL over xGMI);
 *                       RCCL is loaded at run time (dlopen), one distinct device per replica.
 *   GNN_REDUCE_DIRECT : peer-mapped gradient buffers, stream events between the devices, ONE kernel per
 *                       replica that sums all partial gradients in rank order and updates (no collective
 *                       library; replicas may share a device, which is how it is tested on one GPU).
 * Everything that is per net (propagate, loss, argmax, get/set of weights, checkpoint) goes through a
 * replica's own handle, gnn_mlp_dp_replica(h, r, &net) -- borrowed, never destroyed by the caller. */
typedef struct gnn_mlp_dp gnn_mlp_dp_t;
typedef enum { GNN_REDUCE_RCCL = 0, GNN_REDUCE_DIRECT = 1, GNN_REDUCE_DIRECT_RS = 2 } gnn_reducer;
int gnn_mlp_dp_create(const int32_t *dims, int n_dims, int out_kind, int inner_act, int last_act, int loss,
                      int64_t seed, int dtype, const int32_t *devices, int n_dev, int max_batch, int reducer,
                      gnn_mlp_dp_t **out);
int gnn_mlp_dp_destroy(gnn_mlp_dp_t *h);
int gnn_mlp_dp_num_replicas(const gnn_mlp_dp_t *h);
int gnn_mlp_dp_replica(gnn_mlp_dp_t *h, int r, gnn_mlp_t **out);
/* NN:51 gradientStep, sharded over the replicas. */
int gnn_mlp_dp_gradient_step(gnn_mlp_dp_t *h, const double *X, const double *Y, int B, double step,
                             double momentum, int noise);
/* Every replica keeps the whole training set (NNT:28-43): any batch of it can then be sharded in place. */
int gnn_mlp_dp_upload_dataset(gnn_mlp_dp_t *h, const double *X, const double *Y, int64_t N);
int gnn_mlp_dp_gradient_step_range(gnn_mlp_dp_t *h, int64_t first, int B, double step, double momentum,
                                   int noise);
int gnn_mlp_dp_train_range(gnn_mlp_dp_t *h, int64_t first, int B, int n_steps, double step, double momentum);
int gnn_mlp_dp_set_weights(gnn_mlp_dp_t *h, const double *flat);
int gnn_mlp_dp_synchronize(gnn_mlp_dp_t *h);
/* *identical = 1 when every replica holds the same weights, momentum and step count, bit for bit. */
int gnn_mlp_dp_replicas_identical(gnn_mlp_dp_t *h, int *identical);

/* ---- a group of nets of one shape, trained side by side ------------------------------------------
 * The reference is run as SWEEPS: every run of MNISTTrainer is one net trained by NeuralNetTrainer with its own step size,
 * batch size or iteration count, each with Random(1) for its weights (SCE:111) and for its sampler (NNT:42).  (Step sizes and
 * momenta are per member in every training call; batch sizes in gnn_mlp_group_train_sampled_sizes.)  A group holds
 * K = n_members in [1, 16] nets of ONE shape / kind / activations / dtype on ONE device, and ONE copy of the training data;
 * on the two-launch path every launch of a group step serves all members (csrc/group_kernels.h).
 * Member k after any group call is bit for bit (weights, momentum, time) the lone handle created with seeds[k] that made the
 * same calls with steps[k], momenta[k].  Members and group calls share one stream: calls run in the order they are issued. */
typedef struct gnn_mlp_group gnn_mlp_group_t;
/* member k's weights are drawn as gnn_mlp_create(seed = seeds[k]) draws them (appendLayer, SCE:139-156), bit for bit */
int gnn_mlp_group_create(const int32_t *dims, int n_dims, int out_kind, int inner_act, int last_act, int loss,
                         const int64_t *seeds, int n_members, int dtype, int device, int max_batch,
                         gnn_mlp_group_t **out);
int gnn_mlp_group_destroy(gnn_mlp_group_t *g);
int gnn_mlp_group_size(const gnn_mlp_group_t *g);
/* Member k as an ordinary handle -- borrowed, like gnn_mlp_dp_replica: propagate, loss, argmax, count_hits_range, get/set of
 * weights and momentum, checkpoints, gradient_step ... work on it.  gnn_mlp_destroy, gnn_mlp_upload_dataset* and
 * gnn_mlp_set_stream on a member return GNN_ERR_STATE (the group owns its memory, dataset and stream). */
int gnn_mlp_group_member(gnn_mlp_group_t *g, int k, gnn_mlp_t **out);
/* ONE copy of the training data (NNT:28-43), shared by every member; the encodings of gnn_mlp_upload_dataset(_u8) */
int gnn_mlp_group_upload_dataset(gnn_mlp_group_t *g, const double *X, const double *Y, int64_t N);
int gnn_mlp_group_upload_dataset_u8(gnn_mlp_group_t *g, const uint8_t *pixels, const uint8_t *labels, int64_t N);
/* gnn_mlp_train_range for every member on the SAME rows (NNT:62 loop over resident batches); member k steps with steps[k],
 * momenta[k] (SCE:333-339) */
int gnn_mlp_group_train_range(gnn_mlp_group_t *g, int64_t first, int B, int n_steps, const double *steps,
                              const double *momenta);
/* gnn_mlp_train_sampled (NNT:82-90) for every member with ONE sampler's draws -- the reference's runs all sample with
 * Random(1), NNT:42: member k ends where a lone handle ends after train_sampled with a sampler of the same seed.  A batch
 * shortened at a refill (NNT:149-155) is shortened for every member alike.  noise != 0 -> GNN_ERR_UNSUPPORTED (SCE:335). */
int gnn_mlp_group_train_sampled(gnn_mlp_group_t *g, gnn_sampler_t *s, int iterations, int batch, const double *steps,
                                const double *momenta, int noise);
/* 2: every launch of a group step serves all members (the two-launch path); 0: the members are stepped one after another
 * through their own handles (nets off that path, or whose row-block kernel is middle4_kernel) -- same results, no speed-up */
int gnn_mlp_group_launches_per_step(const gnn_mlp_group_t *g);
/* gnn_mlp_train_sampled_observed (NNT:68-72 / 75-79) for every member with ONE sampler's draws:
 * val_loss[i * K + k] = validate(validation_size) of member k after iteration i (iterations x K values).  One readback.
 * The members and the sampler end as after gnn_mlp_group_train_sampled with the same arguments, bit for bit: the validation
 * pass writes no weight, momentum, step count or look-ahead state.  validation_size outside [1, dataset rows] or a null
 * val_loss -> GNN_ERR_BAD_ARG; noise != 0 -> GNN_ERR_UNSUPPORTED. */
int gnn_mlp_group_train_sampled_observed(gnn_mlp_group_t *g, gnn_sampler_t *s, int iterations, int batch,
                                         const double *steps, const double *momenta, int noise,
                                         int validation_size, double *val_loss);
/* 3: two grouped step launches + one grouped validation launch (per block of validation rows) per iteration, the curves summed
 * on the device; 0: member after member, each through gnn_mlp_train_sampled_observed on its own handle (groups of one net, or
 * without grouped step launches) -- column k is then bit for bit the lone handle's curve */
int gnn_mlp_group_observed_launches(const gnn_mlp_group_t *g);
/* gnn_mlp_group_train_sampled / _observed with ONE SAMPLER PER MEMBER: member k ends bit for bit (weights, momentum, time)
 * where the lone handle created with seeds[k] ends after gnn_mlp_train_sampled(samplers[k], iterations, batch, steps[k],
 * momenta[k]); samplers[k] ends where it ends there.  val_loss null: unobserved (validation_size ignored); else
 * val_loss[i * K + k] = validate(validation_size) of member k after iteration i, as gnn_mlp_group_train_sampled_observed.
 * The samplers may be in any state and are independent of one another; their draws are made on up to 8 worker threads.
 * An iteration in which every member's batch has the same size -- every full batch -- is stepped by the two grouped launches;
 * a refill shortens a batch per member (NNT:149-155), and an iteration whose sizes differ is stepped member after member.
 * Refused before any step and any draw: a null or repeated sampler, a sampler whose size differs from the data set, batch not
 * below it (NNT:63), val_loss with validation_size outside [1, rows] -> GNN_ERR_BAD_ARG; noise != 0 -> GNN_ERR_UNSUPPORTED.
 * Groups without grouped launches (gnn_mlp_group_launches_per_step() == 0, one member; observed: gnn_mlp_group_observed_launches()
 * == 0) run member k through gnn_mlp_train_sampled(_observed) with samplers[k]. */
int gnn_mlp_group_train_sampled_each(gnn_mlp_group_t *g, gnn_sampler_t *const *samplers, int iterations, int batch,
                                     const double *steps, const double *momenta, int noise,
                                     int validation_size, double *val_loss);
/* gnn_mlp_group_train_sampled_each with ONE BATCH SIZE PER MEMBER -- the reference's recorded sweep (logs/trainLog.csv rows 1-3:
 * 784-100-50-10, 100 000 iterations, step 0.0042 / 0.0075 / 0.0100 with batch 2 / 4 / 8) as one call.  Member k ends bit for bit
 * (weights, momentum, time) where the lone handle created with seeds[k] ends after gnn_mlp_train_sampled(samplers[k], iterations,
 * batches[k], steps[k], momenta[k]); samplers[k] ends where it ends there.  val_loss null: unobserved; else val_loss[i * K + k] =
 * validate(validation_size) of member k after iteration i, from one readback -- column k bit for bit the lone handle's
 * gnn_mlp_train_sampled_observed curve (behind every grouped step each member is validated by the single-net forward pass).
 * EVERY iteration is stepped by the two grouped launches, member k with its own live row count (csrc/group_kernels.h): a refill
 * that shortens one member's batch (NNT:149-155) changes that member's rows and nothing else, so with equal batches this call
 * also runs a seed-variance study without the member-after-member iterations of gnn_mlp_group_train_sampled_each.
 * gnn_mlp_group_sampled_each_iterations then reports (iterations, 0); (0, iterations) for groups without grouped launches
 * (as above), which run member k through gnn_mlp_train_sampled(_observed) with samplers[k], batches[k].
 * Refused before any step and any draw: null batches, a batches[k] outside [1, max_batch] or not below the data set's rows
 * (NNT:63) -> GNN_ERR_BAD_ARG; everything gnn_mlp_group_train_sampled_each refuses, with its codes. */
int gnn_mlp_group_train_sampled_sizes(gnn_mlp_group_t *g, gnn_sampler_t *const *samplers, int iterations, const int32_t *batches,
                                      const double *steps, const double *momenta, int noise,
                                      int validation_size, double *val_loss);
/* of the LAST gnn_mlp_group_train_sampled_each / _sizes call: iterations stepped by grouped launches / member after member */
int gnn_mlp_group_sampled_each_iterations(const gnn_mlp_group_t *g, int64_t *grouped, int64_t *member_after_member);
int gnn_mlp_group_synchronize(gnn_mlp_group_t *g);
/* Evaluation of a whole group in one pass (csrc/group_eval_kernel.h).
 * 2: one grouped forward launch + one combine launch per block of rows; 0: member after member */
int gnn_mlp_group_eval_launches(const gnn_mlp_group_t *g);
/* rows [first, first + n) of the group's data set, any n: member_hits[k] as gnn_mlp_count_hits_range counts them (MT:159-197),
 * member_loss_sum[k] = sum of calculateLoss over the rows (validate() of NNT:102-113 without its division), *ensemble_hits for the
 * mean output.  Each of the three may be null, not all of them.  One readback. */
int gnn_mlp_group_evaluate_range(gnn_mlp_group_t *g, int64_t first, int64_t n, int64_t *member_hits,
                                 double *member_loss_sum, int64_t *ensemble_hits);
/* the ensemble's propagate() and argmax over the same rows: mean_out is n x d_out (fp64 of the f32 mean), labels has n entries;
 * either may be null, not both */
int gnn_mlp_group_ensemble_range(gnn_mlp_group_t *g, int64_t first, int64_t n, double *mean_out, int32_t *labels);
/* Confusion matrices of the same pass (MT:159-197; the loss pass of NNT:102-113 runs with it and is not returned):
 * member_confusion[(k * d_out + e) * d_out + p] = rows whose expected class (MT:186-188) is e and on which member k's `>=` argmax
 * is p; ensemble_confusion the same for the argmax of the mean output; member_labels[k * n + i] = member k's argmax of row
 * first + i, the labels the counts were made from.  Each of the three may be null, not all of them.  One more launch per
 * block of rows behind the combine kernel (csrc/confusion_kernel.h), one readback; exact integer counts.  Writes no weight,
 * momentum, step count or look-ahead state; each member's deferred host-batch update is applied first. */
int gnn_mlp_group_confusion_range(gnn_mlp_group_t *g, int64_t first, int64_t n, int64_t *member_confusion /* [K][d_out][d_out] */,
                                  int64_t *ensemble_confusion /* [d_out][d_out] */, int32_t *member_labels /* [K][n] */);
/* gnn_mlp_input_gradient_range (NN:27, SCE:207-220, GNN:230-242; SCE:272-278 continued to the input) for every member and for
 * the ensemble: the members run one after the other through their borrowed handles on the group's stream, block by block; the
 * ensemble's gradient is the members' mean formed as gnn_mlp_group_ensemble_range forms the mean output -- f32, member order,
 * one division by (float)K -- and its saliency is summed from that.  member_grad[(k * n + r) * d_0 + i], member_saliency
 * [(k * d_out + e) * d_0 + i]; each of the five may be null, not all of them.  One readback.  Every member's gradient buffer
 * holds its last block's weight gradient afterwards; no weight, momentum, step count or sampler changes. */
int gnn_mlp_group_input_gradient_range(gnn_mlp_group_t *g, int64_t first, int64_t n, double *member_grad /* [K][n][d_0] or null */,
                                       double *ensemble_grad /* [n][d_0] or null */,
                                       double *member_saliency /* [K][d_out][d_0] or null */,
                                       double *ensemble_saliency /* [d_out][d_0] or null */,
                                       int64_t *class_rows /* [d_out] or null */);
/* The group's held-out set (gnn_mlp_upload_held_out*): ONE copy, which the members see through their borrowed handles; the
 * rules of the lone uploads hold for every member. */
int gnn_mlp_group_upload_held_out(gnn_mlp_group_t *g, const double *X, const double *Y, int64_t N);
int gnn_mlp_group_upload_held_out_u8(gnn_mlp_group_t *g, const uint8_t *pixels, const uint8_t *labels, int64_t N);
/* gnn_mlp_group_evaluate_range, _ensemble_range and _confusion_range with the set named (gnn_data_set; MT:159-172 on
 * GNN_SET_HELD_OUT): bit for bit the existing call with GNN_SET_TRAIN, and with GNN_SET_HELD_OUT what it returns on a group with
 * the same weights whose training set is those rows.  The named set never uploaded -> GNN_ERR_STATE; rows outside it, or a
 * `set` that is neither value -> GNN_ERR_BAD_ARG. */
int gnn_mlp_group_evaluate_set_range(gnn_mlp_group_t *g, int set, int64_t first, int64_t n, int64_t *member_hits,
                                     double *member_loss_sum, int64_t *ensemble_hits);
int gnn_mlp_group_ensemble_set_range(gnn_mlp_group_t *g, int set, int64_t first, int64_t n, double *mean_out, int32_t *labels);
int gnn_mlp_group_confusion_set_range(gnn_mlp_group_t *g, int set, int64_t first, int64_t n, int64_t *member_confusion,
                                      int64_t *ensemble_confusion, int32_t *member_labels);
/* gnn_mlp_train_sampled_held_out for every member: trains exactly as gnn_mlp_group_train_sampled_sizes (one sampler and one
 * batch size per member; groups without grouped launches member after member), and at point p column k of point_hits /
 * point_loss ([p * K + k]) and ensemble_hits[p] are bit for bit what gnn_mlp_group_evaluate_set_range(g, GNN_SET_HELD_OUT, 0,
 * held_rows, ..) would return there (MT:159-172 for every member, and the row of MT:241 along the run).  The best point is
 * decided per member; best_weights[k * num_params ..] are member k's weights at best_point[k] (unwritten when that is -1).
 * One keep_best launch per point serves all members.  Refuses what the lone call and gnn_mlp_group_train_sampled_sizes
 * refuse, with their codes. */
int gnn_mlp_group_train_sampled_held_out(gnn_mlp_group_t *g, gnn_sampler_t *const *samplers, int iterations,
                                         const int32_t *batches, const double *steps, const double *momenta, int noise,
                                         int every, int64_t held_rows, int rule,
                                         int64_t *point_hits /* [P][K] */, double *point_loss /* [P][K] */,
                                         int64_t *ensemble_hits /* [P] or null */,
                                         int32_t *best_point /* [K] */, double *best_weights /* [K][num_params] or null */);

/* ---- targets of resident rows ---------------------------------------------------------------------
 * The expected rows of a resident set (gnn_data_set) read back, rewritten in place, and written ON THE DEVICE from a teacher's
 * outputs -- the classic use of an ensemble: train one small net on the ensemble's outputs (csrc/distill.hip,
 * csrc/distill_kernel.h).  Nothing here reallocates a set, touches an input row or changes the look-ahead state: what a handle
 * prepares ahead reads input rows only.  With these calls unused every result is bit for bit what it was. */
/* Y[i * d_out + c] = the fp64 of the f32 expected value the device holds for row first + i.  Works on borrowed handles (a
 * member of a group reads the group's one copy).  A `set` that is neither value, rows outside the set -> GNN_ERR_BAD_ARG; the
 * named set never uploaded -> GNN_ERR_STATE. */
int gnn_mlp_get_targets_range(gnn_mlp_t *h, int set, int64_t first, int64_t n, double *Y /* [n][d_out] */);
/* Rewrites the expected rows [first, first + n) of the named set, converted to f32 exactly as gnn_mlp_upload_dataset converts
 * its Y; every other row, the padding and the inputs stay as they are; no allocation.  Ordered behind everything in flight on
 * the handle's stream; a deferred host-batch update is applied first.  Afterwards the handle behaves bit for bit like one whose
 * set was uploaded with those targets in the first place -- also with a gnn_mlp_hint_next_range pending.  Refusals as above;
 * on a member of a group -> GNN_ERR_STATE (the group call writes the one copy). */
int gnn_mlp_set_targets_range(gnn_mlp_t *h, int set, int64_t first, int64_t n, const double *Y);
int gnn_mlp_group_set_targets_range(gnn_mlp_group_t *g, int set, int64_t first, int64_t n, const double *Y);
/* NN:16 propagate() over rows [first, first + n) of the named set, any n: the output rows of the evaluation pass -- the blocks
 * and launches of gnn_mlp_evaluate_set_range, whose labels are the `>=` argmax (MT:166-168) of these rows, bit for bit --
 * collected on the device and read back once (fp64 of the f32 outputs).  Writes no weight, momentum, step count or look-ahead
 * state.  Works on borrowed handles. */
int gnn_mlp_propagate_set_range(gnn_mlp_t *h, int set, int64_t first, int64_t n, double *out /* [n][d_out] */);
/* Distillation on the device.  For every row r in [first, first + n) of the STUDENT's training set and every class c:
 *   y'[r][c] = keep_f * y[r][c] + (1.f - keep_f) * t[r][c]      in f32, keep_f = (float)keep, no fused multiply-add,
 * t = the teacher's output on the student's resident input row r: for a net what gnn_mlp_propagate_set_range returns on those
 * rows, for a group the mean output as gnn_mlp_group_ensemble_range forms it (f32, member order, one division by (float)K;
 * groups off the grouped evaluation plan run member after member into the same blend).  The teacher runs its usual evaluation
 * pass with the student's rows as its data set, and one more launch per block of rows blends into the student's expected rows.
 * keep == 1 leaves every bit unchanged, keep == 0 makes the rows bit for bit the f32 teacher output; padding stays zero.
 * Synchronous: the student's stream is synchronised before the teacher's stream writes, the teacher's before the call returns.
 * The teacher's weights, momentum, step count and look-ahead state are untouched (its deferred host-batch update is applied
 * first); teacher == student is allowed.  Hidden layers, depth and output kind may differ.  Refused before any work: a null
 * handle, keep outside [0, 1] or NaN, rows outside the set, teacher and student differing in dims[0], dims[L-1], inner
 * activation, dtype or device (the message names which) -> GNN_ERR_BAD_ARG; no training set on the student, a student that is
 * a member of a group or a replica of a gnn_mlp_dp_t -> GNN_ERR_STATE.
 * Hit counts on a set whose targets are no longer one-hot follow the expected-class rule (the last exact 1.0, else class 0):
 * accuracy on the training set means nothing after this call; the held-out set is untouched and stays the measure. */
int gnn_mlp_distill_range(gnn_mlp_t *student, gnn_mlp_t *teacher, int64_t first, int64_t n, double keep);
int gnn_mlp_group_distill_range(gnn_mlp_t *student, gnn_mlp_group_t *teachers, int64_t first, int64_t n, double keep);

/* ---- adversarial rows (fast gradient sign) --------------------------------------------------------
 * The perturbation x' = clip(x + eps * sign(g), lo, hi), g = d calculateLoss(x, y) / d x (NN:27, SCE:207-220, GNN:230-242; the
 * gradient gnn_mlp_input_gradient_range returns), formed ON THE DEVICE from the rows it holds (csrc/adversarial.hip; the kernel:
 * csrc/input_grad_kernel.h, fgsm_kernel).  Per element, in f32 with every operation rounded on its own (no fused multiply-add):
 *   a' = min(max(a + eps_f * s, lo_f), hi_f),   s = (g > 0) - (g < 0)
 * with g bit for bit the value gnn_mlp_input_gradient_range returns for the element: s(0) = 0, a NaN g leaves the element
 * unperturbed; eps == 0 returns rows inside [lo, hi] bit for bit.  The device holds a = f(x), not x (the reference applies f to
 * the raw input too, SCE:183-186), so the calls serve the inner activations that are the identity on non-negative values --
 * leaky ReLU (MT:235), ReLU, identity -- with 0 <= lo <= hi, and it is the caller's PRECONDITION, not checked, that the rows are
 * non-negative (rows uploaded with gnn_mlp_upload_dataset_u8 always are).  Lone nets of either dtype on every plan; a member of a
 * group or a replica of a gnn_mlp_dp_t -> GNN_ERR_STATE.  A sigmoid or tanh inner activation -> GNN_ERR_UNSUPPORTED; eps
 * negative or not finite, lo < 0, hi < lo, a NaN bound -> GNN_ERR_BAD_ARG.  A deferred host-batch update is applied first.
 * The two range calls work in blocks of at most max_batch rows, each the handle's gradient computation without an update plus
 * one launch, with no host work between blocks and one readback; they change no weight, momentum, step count or sampler,
 * overwrite the host-batch staging rows, leave the gradient buffer with the last block's weight gradient like
 * gnn_mlp_compute_gradient*, and (training set) leave the look-ahead state as gnn_mlp_compute_gradient_range on the last block
 * leaves it.  The named set never uploaded -> GNN_ERR_STATE; rows outside it, a `set` that is neither value -> GNN_ERR_BAD_ARG. */
/* the perturbed rows themselves (fp64 of the f32 values) */
int gnn_mlp_fgsm_set_range(gnn_mlp_t *h, int set, int64_t first, int64_t n, double eps, double lo, double hi,
                           double *X_adv /* [n][d_0] */);
/* Robust accuracy and loss (testOnTestData / testOnTrainingData, MT:159-197, and validate(), NNT:102-113, on the perturbed
 * rows): per block the perturbation, then the forward pass and the reductions of gnn_mlp_evaluate_set_range -- the `>=` argmax
 * (MT:166-168) against the expected class, the loss summed block after block into one slot.  Either output may be null, not both. */
int gnn_mlp_evaluate_fgsm_set_range(gnn_mlp_t *h, int set, int64_t first, int64_t n, double eps, double lo, double hi,
                                    int64_t *hits, double *loss_sum);
/* Adversarial training: the loop of gnn_mlp_train_sampled (NNT:60-92; the same draws, chunks and refusals, the sampler left where
 * that call leaves it) in which every iteration trains on the perturbation of its own batch against the weights of that moment:
 * the drawn rows gathered into the staging rows, the gradient computation without an update, the perturbation in place, then the
 * step (SCE:299-345) on the perturbed rows with the rows' own targets.  The step count advances once per iteration. */
int gnn_mlp_train_sampled_fgsm(gnn_mlp_t *h, gnn_sampler_t *s, int iterations, int batch, double step, double momentum, double eps,
                               double lo, double hi);

/* ---- adversarial rows (projected gradient descent; BIM without the random start) ------------------
 * The iterated, projected form of the perturbation above (csrc/adversarial.hip; the kernels: csrc/input_grad_kernel.h, pgd_kernel
 * and pgd_start_kernel).  The current iterate is a, the ORIGIN x0 is the resident row, g the input gradient of the current weights
 * at a, formed exactly as gnn_mlp_input_gradient forms it.  All arithmetic is f32, every operation rounded on its own (no fused
 * multiply-add); eps_f, alpha_f, lo_f, hi_f are the f32 values of the call's doubles.  One step:
 *   s  = (g > 0) - (g < 0)                        s(0) = 0, a NaN g leaves s = 0
 *   v  = a + alpha_f * s
 *   w  = min(max(v, x0 - eps_f), x0 + eps_f)      the ball around the ORIGIN, each bound one rounding
 *   a' = min(max(w, lo_f), hi_f)                  the box last
 * The box comes last: a row outside [lo, hi] ends inside it, as with the one-step call, and steps == 1, alpha == eps, no random
 * start is bit for bit gnn_mlp_fgsm_set_range's result.  After `steps` steps the result is a_T; steps == 0 is allowed and returns
 * the start rows clipped to the box.
 * Random start: start_seed < 0 starts at x0 (the first step then moves x0 itself, unclipped).  0 <= start_seed < 2^31 starts at
 *   mix(u):  u ^= u >> 16;  u *= 0x7feb352d;  u ^= u >> 15;  u *= 0x846ca68b;  u ^= u >> 16          (uint32, wrapping)
 *   r = mix(mix(mix(seed) + n) ^ R),   h = mix(r + 0x9E3779B9 * c),   u = float(h >> 8) * 2^-23 - 1   (exact, in [-1, 1))
 *   a_0 = min(max(x0 + eps_f * u, lo_f), hi_f)                                                         (two roundings, then the box)
 * with R the row's index IN ITS RESIDENT SET (first + ... for the range calls, the drawn dataset index in training), c the
 * column, n = 0 for the range calls and the iteration's number within the call in training.  The start cannot leave the ball
 * (rounding is monotonic).
 * Domain and refusals are the one-step calls', through the same check (lone nets, the three inner activations, 0 <= lo <= hi, eps
 * finite and not negative, non-negative rows as the caller's precondition); in addition alpha negative or not finite, steps < 0
 * or > 1024, start_seed >= 2^31 -> GNN_ERR_BAD_ARG.
 * Per block of at most max_batch rows: the start (pgd_start_kernel into the staging rows; none when start_seed < 0 and
 * steps >= 1, the first step then reads the resident rows directly), then per step the handle's gradient computation without an
 * update on the current rows and pgd_kernel in place, the origin read from the resident rows.  No host work and no
 * synchronisation between steps or blocks.  What the range calls overwrite and leave is what the one-step range calls do; the
 * look-ahead state is left as the last gradient computation leaves it -- gnn_mlp_compute_gradient_range on the last block when
 * steps == 1 on the training set without a start, a gradient computation on a host batch otherwise. */
/* the attacked rows themselves (fp64 of the f32 values) */
int gnn_mlp_pgd_set_range(gnn_mlp_t *h, int set, int64_t first, int64_t n, double eps, double alpha, int steps, int64_t start_seed,
                          double lo, double hi, double *X_adv /* [n][d_0] */);
/* Robust hits and loss with the reductions of gnn_mlp_evaluate_fgsm_set_range.  curve == 0: one entry, the state after step
 * `steps`.  curve == 1: steps + 1 entries, entry t the state after t steps, entry 0 the start rows (one more forward pass and two
 * reductions per step and block; one fill, one readback).  Entry t is bit for bit what the call with steps = t, curve = 0
 * returns.  Either output may be null, not both; curve other than 0 / 1 -> GNN_ERR_BAD_ARG. */
int gnn_mlp_evaluate_pgd_set_range(gnn_mlp_t *h, int set, int64_t first, int64_t n, double eps, double alpha, int steps,
                                   int64_t start_seed, double lo, double hi, int curve, int64_t *hits, double *loss_sum);
/* Adversarial training with the iterated attack: gnn_mlp_train_sampled_fgsm's loop, every iteration a gather of the drawn rows,
 * the start, `steps` x (gradient computation without an update, pgd_kernel with the origin read from the resident training rows
 * through the iteration's index vector), then the step on the attacked rows.  Draws, chunks, refusals and the sampler's end state
 * are gnn_mlp_train_sampled's; the step count advances once per iteration. */
int gnn_mlp_train_sampled_pgd(gnn_mlp_t *h, gnn_sampler_t *s, int iterations, int batch, double step, double momentum, double eps,
                              double alpha, int steps, int64_t start_seed, double lo, double hi);

/* ---- integrated gradients -----------------------------------------------------------------------
 * The attribution of calculateLoss to the inputs along the straight path from a baseline to the row (csrc/input_grad.hip; the
 * kernels: csrc/input_grad_kernel.h, intgrad_kernel, intgrad_start_kernel, intgrad_delta_kernel).  x0 is the resident row, b_f and
 * m_f the f32 values of `baseline` and `steps` = m, g(a) the input gradient of the current weights at a, formed exactly as
 * gnn_mlp_input_gradient forms it.  All arithmetic is f32, every operation rounded on its own.  The path points are midpoints,
 * alpha_k = (float)((k + 0.5) / m), formed in double and rounded once, k = 0 .. m-1:
 *   d    = x0 - b_f                              one rounding
 *   a_k  = b_f + alpha_k * d                     product, then sum
 *   S_0  = g(a_0);   S_k = S_{k-1} + g(a_k)      step order
 *   IG   = d * (S_{m-1} / m_f)                   division, then product
 * Domain: the adversarial calls', through the same check -- lone nets (GNN_ERR_STATE for a member of a group or a replica),
 * leaky ReLU, ReLU or identity inside (GNN_ERR_UNSUPPORTED otherwise: the device holds f(x)), non-negative rows as the caller's
 * precondition.  baseline is one scalar, finite and >= 0 (0: the black image), 1 <= steps <= 1024; GNN_ERR_BAD_ARG otherwise.
 * Every a_k is then >= 0 (fl(x0 - b_f) >= -b_f and rounding is monotonic), a valid f(x).  A baseline ROW, groups, ensembles,
 * sampled and training forms are not served.
 * Per block of at most max_batch rows: the first point into the staging rows, then m x (the handle's gradient computation
 * without an update on the staging rows, intgrad_kernel in place); the block's attributions end in the input-gradient buffer.
 * No host work and no synchronisation between steps or blocks; one fill, one readback.
 * Outputs, any of them null, not all: the attributions (fp64 of the f32 values); maps[c][i], the sum of |IG[.][i]| over the rows
 * whose expected class (MT:186-188) is c, in fp64 in row order, and class_rows[c], their number (the reductions of
 * gnn_mlp_input_gradient_range); delta[r] = sum_i IG[r][i] - (calculateLoss(x0_r) - calculateLoss(baseline row)), the
 * completeness check: the row's cells summed in fp64 in column order, the two f32 per-row losses from one forward pass over the
 * block's rows and one over baseline rows (two more forward passes per block).
 * The call applies a pending host-batch update first and changes no weight, momentum, step count, sampler or look-ahead state
 * (its gradient computations are those of a host batch).  It overwrites the staging rows, activations, deltas and the
 * input-gradient buffer, and like gnn_mlp_compute_gradient* leaves the gradient buffer with its last block's weight gradient
 * (at the last path point). */
int gnn_mlp_integrated_gradients_set_range(gnn_mlp_t *h, int set, int64_t first, int64_t n, int steps, double baseline,
                                           double *attributions /* [n][d_0] */, double *maps /* [d_out][d_0] */,
                                           int64_t *class_rows /* [d_out] */, double *delta /* [n] */);

/* ---- shape specialisation ---------------------------------------------------------------------
 * The per-row-block kernel of the fused small-net path is a template over the net's shape; with
 * compile-time layer sizes it is ~1.5x faster than with sizes read from kernel arguments.
 * gnn_mlp_specialize instantiates it for THIS net at run time (hiprtc, ~0.4 s once per shape and
 * process); a handle does it by itself at its 16th gradient computation or when a long training
 * call (>= 64 steps) starts; env GNN_MLP_JIT=0 turns it off.  Results are bitwise identical
 * either way.
 * gnn_mlp_specialization: 0 = generic kernels (sizes from arguments, or the net does not take
 * the fused path), 1 = prebuilt instantiation (the two MNIST shapes BASELINE.json names),
 * 2 = instantiated at run time. */
int gnn_mlp_specialize(gnn_mlp_t *h);
int gnn_mlp_specialization(const gnn_mlp_t *h);
/* Kernel launches of one gradientStep inside a training loop on this net: 2 = the two-launch path
 * (row-block kernel + tile-owner kernel, csrc/tile_step_kernel.h), 3 = first layer / row-block kernel /
 * gradient+update, 0 = per-layer GEMMs (the count then depends on the layer count). */
int gnn_mlp_step_launches(const gnn_mlp_t *h);
/* The row-block kernel of the two-launch TRAINING step (csrc/rowblock_kernel.h): 0 = not taken (bf16, a plan that does not
 * fit, GNN_MLP_ROWBLOCK=0: the step then uses middle4_kernel), 1 = runtime-shape instantiation, 2 = prebuilt for the shape,
 * 3 = instantiated at run time for the shape (gnn_mlp_specialize / the 16th step). */
int gnn_mlp_rowblock_state(const gnn_mlp_t *h);
/* The tile-owner kernel's TRAINING launch (gradient + update + next slabs) of this net: 0 = one tile per workgroup, n > 0 = the
 * merged map (csrc/tile_step_kernel.h, make_merged_tile_map: light tiles share a workgroup, no CU runs two) in a grid of n
 * workgroups.  0 for bf16, group members, a net with more units than CUs, off the row-block kernel's path, GNN_MLP_TILE_MERGE=0. */
int gnn_mlp_tile_merge_state(const gnn_mlp_t *h);
/* Why gnn_mlp_step_launches() is not 2 for this net ("" when it is): the decision gnn_mlp_create took (layer count,
 * LDS budget, slab count, a failed allocation, a GNN_MLP_* development switch).  The string lives as long as the handle. */
const char *gnn_mlp_plan_note(const gnn_mlp_t *h);

/* ---- measurement support (bench.py) -------------------------------------------------------
 * Mean duration in microseconds of the kernel class `which` over the launches since the last
 * reset.  Kernel classes are timed with the dispatch's own begin/end timestamps
 * (hipExtLaunchKernel start/stop events on the handle's stream), i.e. the quantity rocprofv3's
 * kernel trace reports; timing must be enabled first. */
typedef enum {
    GNN_K_FWD_GEMM0 = 0,  /* first forward GEMM  (B x d_0 x d_1), as its own launch (inference; start of a step chain) */
    GNN_K_GRAD_GEMM0 = 1, /* weight-gradient kernel (d_0 x d_1 x B ...): with the fused update, and on the two-launch
                             path with the next batch's first-layer product */
    GNN_K_STEP = 2,       /* one whole gradient step (events recorded around the launches) */
    GNN_K_MIDDLE = 3,     /* fused path only: the per-row-block kernel between A_1 and delta_1 */
    GNN_K_UPDATE = 4      /* data-parallel path: the momentum update after the all-reduce */
} gnn_kernel_class;
int gnn_mlp_timing_enable(gnn_mlp_t *h, int on);
int gnn_mlp_timing_read(gnn_mlp_t *h, int which, double *mean_us, int64_t *count);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* GNN_MLP_H */
