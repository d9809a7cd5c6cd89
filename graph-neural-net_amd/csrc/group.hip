// group.hip -- a group of nets of one shape trained side by side (include/gnn_mlp.h, gnn_mlp_group_*): hyperparameter sweeps,
// ensembles and seed-variance runs in one call.
//
// The members are ordinary handles (abi.hip) whose create-time device buffers are carved out of ONE arena, member k's slice at
// member 0's + k * S: every member makes the same allocations of the same sizes, so the pointer rule of group_kernels.h turns
// member 0's kernel arguments into member k's.  A group step then drives MEMBER 0's control path (plan.hip: chain_gradient,
// launch_small.hip) with GroupLaunch set, which turns each of its two launches into the grouped launch -- there is no second
// copy of the chain logic.  What a step reads and every member shares -- the dataset, the device index ring of a sampled
// call -- is member 0's and lies outside the arena.  (A call with one sampler per member keeps K index rings in one region
// outside the arena, a second relocatable range; a call with one BATCH SIZE per member, gnn_mlp_group_train_sampled_sizes, hands
// the grouped launches every member's own row count: the end of this file.)  Nets off the two-launch path are stepped one member
// after another through their own handles: the same results, no speed-up.
//
// Every training entry point that launches for the group does so through ONE scaffold, GroupedCall::run, the only place that
// spells enter_grouped / GroupScope / leave_grouped.  Its rules: leave_grouped also runs when the loop failed (the steps it did
// take are the members' too); everything a call allocates is allocated before enter_grouped; the counters of a call with one
// sampler per member are zeroed before the decision to go member after member; and the GroupScope ends before the members'
// state is copied.  An entry point adds its checks, its observer and its fallback, nothing of the above.
#include "handle.h"

#include <algorithm>
#include <memory>

using namespace gnn;
using namespace gnn::host;

namespace {

void free_group(gnn_mlp_group *g) {
    if (g->stream) (void)hipStreamSynchronize(g->stream);
    free_group_eval(g);
    for (gnn_mlp *h : g->m) if (h) destroy_handle(h);
    if (g->arena) (void)hipFree(g->arena);
    if (g->stream) (void)hipStreamDestroy(g->stream);
    delete g;
}

static_assert(kGroupSizesMax == GROUP_MAX, "group_sizes.h and group_kernels.h: one member count");

// Before a grouped call: every member's deferred update is applied, and member 0's look-ahead state (lookahead.h) -- which the
// grouped launches act on for everyone -- must describe every member: member k holds it with its own pointers and, after a call
// with one batch size per member, its own sizes (group_sizes.h: the group's record of them).  If it does not (a member was
// stepped alone), all of it is dropped: forgetting keeps results bitwise, it only costs a forward-only launch.
int enter_grouped(gnn_mlp_group *g) {
    for (gnn_mlp *h : g->m) TRY(check_handle(h));
    const Lookahead &l0 = g->m[0]->la;
    // (sizes that differ between the members describe batches of a sized call's index region, which is gone: never live)
    bool same = g->sizes.describes(l0) && (g->sizes.is_uniform(g->K) || (!l0.slab_valid && !l0.have_next));
    for (int k = 1; k < g->K && same; k++) same = g->sizes.member_view(l0, g->arena, g->S, k) == g->m[k]->la;
    if (!same)
        for (int k = 0; k < g->K; k++) { g->m[k]->la = g->m[0]->la.rebased(g->arena, g->S, k); g->m[k]->la.forget(); } // (one staging buffer index for all)
    if (!same) g->sizes.uniform(g->K, g->m[0]->la);
    return GNN_OK;
}
// After it: member 0's step count and look-ahead state, moved to each member.  (idx_lo, idx_S: the index region of a call
// with one sampler per member while it is live -- lookahead.h.  sizes: the members' own batch sizes, a sized call; else member
// 0's hold for all.)
void leave_grouped(gnn_mlp_group *g, int steps_done, const char *idx_lo = nullptr, size_t idx_S = 0, const GroupSizes *sizes = nullptr) {
    if (sizes) g->sizes = *sizes;
    else g->sizes.uniform(g->K, g->m[0]->la);
    for (int k = 1; k < g->K; k++) {
        g->m[k]->time += steps_done;
        g->m[k]->la = g->sizes.member_view(g->m[0]->la, g->arena, g->S, k, idx_lo, idx_S);
    }
}

struct GroupScope { // member 0 launches for the group while this lives
    gnn_mlp *h;
    GroupScope(gnn_mlp *h_, const GroupLaunch *gl) : h(h_) { h->grp = gl; }
    ~GroupScope() { h->grp = nullptr; }
};

int group_launch(const gnn_mlp_group *g, const double *steps, const double *momenta, GroupLaunch *gl) {
    gl->K = g->K;
    gl->arena_lo = g->arena;
    gl->S = g->S;
    gl->rb_fn = g->rb_fn;
    gl->rb_fn_sized = g->rb_fn_sized;
    for (int k = 0; k < g->K; k++) { gl->step[k] = steps[k]; gl->momentum[k] = momenta[k]; }
    return GNN_OK;
}

int check_group(gnn_mlp_group *g) {
    if (!g) return fail(GNN_ERR_BAD_ARG, "null group");
    HIP_TRY(hipSetDevice(g->device));
    return GNN_OK;
}
int check_per_member(const gnn_mlp_group *g, const double *steps, const double *momenta) {
    if (!steps || !momenta) return fail(GNN_ERR_BAD_ARG, "steps and momenta: one value per member, not null");
    for (int k = 0; k < g->K; k++)
        if (!(steps[k] > 0)) return fail(GNN_ERR_BAD_ARG, "step must be positive (SCE:301)");
    return GNN_OK;
}

// One call's grouped launches (the head of this file): run() hands `loop` the GroupLaunch under which member 0 launches for the
// group, and whatever status the loop returns -- the steps it took are taken -- moves member 0's step count and look-ahead
// state to the members.  The GroupLaunch lives in run() alone, so what points into it (EachMember, SizedMembers below) can only
// be made inside the loop and is gone before it; what such an object has to say to leave_grouped it writes to `mixed` / `track`.
struct GroupedCall {
    gnn_mlp_group *g;
    bool sized = false;   // one batch size per member: the launches take every member's row count, the members leave with `track`
    bool counted = false; // one sampler per member: g->each_grouped / each_mixed say how the iterations were stepped
    int64_t mixed = 0;    // iterations the loop stepped member after member, through the members' own handles: step counts included
    GroupSizes track;     // sized: member k's sizes of the batches member 0's state names (valid once enter_grouped has run)

    template <class Loop> int run(const double *steps, const double *momenta, Loop &&loop) {
        TRY(enter_grouped(g));
        GroupLaunch gl;
        TRY(group_launch(g, steps, momenta, &gl));
        gl.sized = sized;
        gnn_mlp *h0 = g->m[0];
        const int t0 = h0->time;
        int rc;
        {
            GroupScope scope(h0, &gl);
            rc = loop(gl);
        }
        const int done = h0->time - t0;
        // (a mixed iteration advanced every member's step count through its own handle: only the grouped ones are member 0's alone)
        leave_grouped(g, done - (int)mixed, nullptr, 0, sized ? &track : nullptr);
        if (counted) { g->each_mixed = mixed; g->each_grouped = done - mixed; }
        return rc;
    }
};

// Member k trained through its own handle, as the lone net it is.  With a curve (val_loss, [iterations][K]): column k is the lone
// handle's curve.
int member_sampled(gnn_mlp_group *g, int k, gnn_sampler_t *s, int iterations, int batch, double step, double momentum, int noise,
                   int validation_size, double *val_loss) {
    const int K = g->K;
    gnn_mlp *h = g->m[(size_t)k];
    if (!val_loss) return gnn_mlp_train_sampled(h, s, iterations, batch, step, momentum, noise);
    std::vector<double> col((size_t)iterations);
    TRY(gnn_mlp_train_sampled_observed(h, s, iterations, batch, step, momentum, noise, validation_size, col.data()));
    for (int i = 0; i < iterations; i++) val_loss[(size_t)i * K + k] = col[(size_t)i];
    return GNN_OK;
}
// The two ways member after member.  ONE sampler: every member draws what the sampler draws from its state at the call -- it is
// rewound for each and ends where the last member's run leaves it ...
int members_one_sampler(gnn_mlp_group *g, gnn_sampler_t *s, int iterations, int batch, const double *steps, const double *momenta,
                        int noise, int validation_size = 0, double *val_loss = nullptr) {
    std::unique_ptr<gnn_sampler_t, int (*)(gnn_sampler_t *)> start(sampler_copy(s), gnn_sampler_destroy);
    for (int k = 0; k < g->K; k++) {
        if (k) sampler_assign(s, start.get());
        TRY(member_sampled(g, k, s, iterations, batch, steps[k], momenta[k], noise, validation_size, val_loss));
    }
    return GNN_OK;
}
// ... a sampler per member: each with its own sampler and batch size, never rewound.
int members_own_samplers(gnn_mlp_group *g, gnn_sampler_t *const *samplers, int iterations, const int *batches, const double *steps,
                         const double *momenta, int noise, int validation_size = 0, double *val_loss = nullptr) {
    for (int k = 0; k < g->K; k++)
        TRY(member_sampled(g, k, samplers[k], iterations, batches[k], steps[k], momenta[k], noise, validation_size, val_loss));
    return GNN_OK;
}

// What a call with one sampler per member refuses about them, member k against its own sampler and batch size; `val_loss`: the
// curve request.  (The callers that take an ARRAY of batch sizes refuse a null one themselves, between "samplers is null" and the
// samplers' own checks: `samplers && !batches` in front of this.)
int check_member_samplers(gnn_mlp_group *g, gnn_sampler_t *const *samplers, int iterations, const int *batches, const double *steps,
                          int noise, int validation_size, const double *val_loss) {
    const int K = g->K;
    if (!samplers) return fail(GNN_ERR_BAD_ARG, "samplers is null");
    for (int k = 0; k < K; k++) if (!samplers[k]) return fail(GNN_ERR_BAD_ARG, "null sampler");
    for (int k = 0; k < K; k++)
        for (int j = 0; j < k; j++)
            if (samplers[j] == samplers[k]) return fail(GNN_ERR_BAD_ARG, "the same sampler for two members: every member draws from its own");
    for (int k = 0; k < K; k++) TRY(train_sampled_checks(g->m[k], samplers[k], iterations, batches[k], steps[k], noise));
    if (val_loss && (validation_size <= 0 || validation_size > g->m[0]->dataset_n)) return fail(GNN_ERR_BAD_ARG, "validation size outside the dataset (NNT:104)");
    return GNN_OK;
}

} // namespace

extern "C" {

int gnn_mlp_group_create(const int32_t *dims, int n_dims, int out_kind, int inner_act, int last_act, int loss,
                         const int64_t *seeds, int n_members, int dtype, int device, int max_batch,
                         gnn_mlp_group_t **out) { return guarded([&]() -> int {
    if (!out) return fail(GNN_ERR_BAD_ARG, "out is null");
    *out = nullptr;
    if (n_members < 1 || n_members > GROUP_MAX) return fail(GNN_ERR_BAD_ARG, "a group holds 1 to 16 nets");
    if (!seeds) return fail(GNN_ERR_BAD_ARG, "seeds is null");
    // the record pass: one member created as gnn_mlp_create creates it (every argument checked there), its allocations counted
    size_t S = 0;
    {
        ArenaCarve rec; rec.record = true;
        gnn_mlp *probe = nullptr;
        t_arena = &rec;
        const int rc = create_handle(dims, n_dims, out_kind, inner_act, last_act, loss, seeds[0], dtype, device, max_batch, nullptr, &probe);
        t_arena = nullptr;
        if (rc != GNN_OK) return rc;
        destroy_handle(probe);
        S = (rec.used + 255) & ~(size_t)255;
    }
    std::unique_ptr<gnn_mlp_group, void (*)(gnn_mlp_group *)> g(new gnn_mlp_group(), free_group);
    g->K = n_members; g->device = device; g->S = S;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking));
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&g->arena), S * (size_t)n_members));
    g->m.assign((size_t)n_members, nullptr);
    for (int k = 0; k < n_members; k++) {
        ArenaCarve carve; carve.base = g->arena + (size_t)k * S; carve.cap = S;
        t_arena = &carve;
        const int rc = create_handle(dims, n_dims, out_kind, inner_act, last_act, loss, seeds[k], dtype, device, max_batch, g->stream, &g->m[k]);
        t_arena = nullptr;
        if (rc != GNN_OK) return rc;
        g->m[k]->group = g.get();
        if ((carve.used + 255) / 256 * 256 != S) return fail(GNN_ERR_STATE, "the members' allocations differ");
    }
    gnn_mlp *h0 = g->m[0];
    if (h0->chain && h0->rb) {
        g->rb_fn = rb_group_function(h0);
        if (g->rb_fn && hipFuncSetAttribute(g->rb_fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h0->rb_lds_bytes) != hipSuccess) {
            (void)hipGetLastError();
            g->rb_fn = nullptr;
        }
        // (the sized twin, for calls with one batch size per member: both or neither)
        g->rb_fn_sized = g->rb_fn ? rb_group_sized_function(h0) : nullptr;
        if (g->rb_fn_sized && hipFuncSetAttribute(g->rb_fn_sized, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h0->rb_lds_bytes) != hipSuccess) {
            (void)hipGetLastError();
            g->rb_fn_sized = nullptr;
        }
        g->grouped = g->rb_fn != nullptr && g->rb_fn_sized != nullptr;
    }
    plan_group_eval(g.get());
    HIP_TRY(hipStreamSynchronize(g->stream));
    *out = g.release();
    return GNN_OK;
}); }

int gnn_mlp_group_destroy(gnn_mlp_group_t *g) { return guarded([&]() -> int {
    if (!g) return GNN_OK;
    (void)hipSetDevice(g->device);
    free_group(g);
    return GNN_OK;
}); }

int gnn_mlp_group_size(const gnn_mlp_group_t *g) { return g ? g->K : -1; }

int gnn_mlp_group_member(gnn_mlp_group_t *g, int k, gnn_mlp_t **out) { return guarded([&]() -> int {
    if (!g || !out) return fail(GNN_ERR_BAD_ARG, "null argument");
    if (k < 0 || k >= g->K) return fail(GNN_ERR_BAD_ARG, "member index out of range");
    *out = g->m[(size_t)k];
    return GNN_OK;
}); }

int gnn_mlp_group_launches_per_step(const gnn_mlp_group_t *g) { return !g ? -1 : g->grouped ? 2 : 0; }

int gnn_mlp_group_synchronize(gnn_mlp_group_t *g) { return guarded([&]() -> int {
    TRY(check_group(g));
    return gnn_mlp_synchronize(g->m[0]); // (one stream for all members)
}); }

// member 0 uploads (and owns) the data; the others borrow its buffers
static int share_dataset(gnn_mlp_group *g) {
    gnn_mlp *h0 = g->m[0];
    for (int k = 1; k < g->K; k++) {
        gnn_mlp *h = g->m[k];
        h->DX = h0->DX; h->DY = h0->DY; h->DXb = h0->DXb; h->dataset_n = h0->dataset_n;
        h->shared_dataset = true;
        h->la.rows_renamed(); // (they name rows of the old dataset)
    }
    return GNN_OK;
}

int gnn_mlp_group_upload_dataset(gnn_mlp_group_t *g, const double *X, const double *Y, int64_t N) { return guarded([&]() -> int {
    TRY(check_group(g));
    for (gnn_mlp *h : g->m) TRY(check_handle(h));
    TRY(upload_dataset_f64(g->m[0], X, Y, N));
    return share_dataset(g);
}); }

int gnn_mlp_group_upload_dataset_u8(gnn_mlp_group_t *g, const uint8_t *pixels, const uint8_t *labels, int64_t N) { return guarded([&]() -> int {
    TRY(check_group(g));
    for (gnn_mlp *h : g->m) TRY(check_handle(h));
    TRY(upload_dataset_u8(g->m[0], pixels, labels, N));
    return share_dataset(g);
}); }

// the held-out set: member 0's too, borrowed by the others -- no look-ahead state names its rows
static int share_held(gnn_mlp_group *g) {
    for (int k = 1; k < g->K; k++) { g->m[k]->held = g->m[0]->held; g->m[k]->shared_held = true; }
    return GNN_OK;
}

int gnn_mlp_group_upload_held_out(gnn_mlp_group_t *g, const double *X, const double *Y, int64_t N) { return guarded([&]() -> int {
    TRY(check_group(g));
    for (gnn_mlp *h : g->m) TRY(check_handle(h, false));
    const int rc = upload_dataset_f64(g->m[0], X, Y, N, GNN_SET_HELD_OUT);
    share_held(g); // (after a failed upload too: the old set is gone for every member)
    return rc;
}); }

int gnn_mlp_group_upload_held_out_u8(gnn_mlp_group_t *g, const uint8_t *pixels, const uint8_t *labels, int64_t N) { return guarded([&]() -> int {
    TRY(check_group(g));
    for (gnn_mlp *h : g->m) TRY(check_handle(h, false));
    const int rc = upload_dataset_u8(g->m[0], pixels, labels, N, GNN_SET_HELD_OUT);
    share_held(g);
    return rc;
}); }

int gnn_mlp_group_train_range(gnn_mlp_group_t *g, int64_t first, int B, int n_steps, const double *steps,
                              const double *momenta) { return guarded([&]() -> int {
    TRY(check_group(g));
    TRY(check_per_member(g, steps, momenta));
    gnn_mlp *h0 = g->m[0];
    TRY(train_range_checks(h0, first, B, n_steps, steps[0]));
    if (g->K == 1 || !g->grouped) { // one member after another, each through its own handle
        for (int k = 0; k < g->K; k++) TRY(gnn_mlp_train_range(g->m[(size_t)k], first, B, n_steps, steps[k], momenta[k]));
        return GNN_OK;
    }
    return GroupedCall{g}.run(steps, momenta, [&](GroupLaunch &) { return train_range_steps(h0, first, B, 0, n_steps, steps[0], momenta[0]); });
}); }

int gnn_mlp_group_train_sampled(gnn_mlp_group_t *g, gnn_sampler_t *s, int iterations, int batch, const double *steps,
                                const double *momenta, int noise) { return guarded([&]() -> int {
    TRY(check_group(g));
    TRY(check_per_member(g, steps, momenta));
    gnn_mlp *h0 = g->m[0];
    TRY(train_sampled_checks(h0, s, iterations, batch, steps[0], noise));
    if (g->K == 1 || !g->grouped) return members_one_sampler(g, s, iterations, batch, steps, momenta, noise);
    return GroupedCall{g}.run(steps, momenta, [&](GroupLaunch &) { return train_sampled_run(h0, &s, 1, iterations, &batch, steps[0], momenta[0], noise, nullptr, nullptr); });
}); }

/* The observed loop (NNT:68-72 / 75-79) of a group: the sampled loops with, behind every step and still under the
 * GroupScope, ONE launch of the forward kernel's validation form per block of validation rows (group_eval.hip) -- the members'
 * per-row losses of iteration i go to row i mod M of a matrix [M][K][stride], which ONE launch of group_curve_sum_kernel turns
 * into d_val[i][k] whenever it is full and behind the last step.  Everything is allocated and checked before the first step. */
namespace {
constexpr int kCurveRows = 256;
// What surrounds an observer that leaves the members' validation loss SUMS on the device (this one, MemberValidation below): its
// buffers, made in front of the first step, and the sums' way to the caller's curve.
struct CurveObserver : SampledObserver {
    gnn_mlp_group *g; int validation_size, iterations; int64_t stride;
    float *d_rows; double *d_val;
    DevScratch rows, val;
    // n_rows: the vectors of `stride` per-row losses the observer keeps (0: none, d_rows null); d_val: iterations * K sums
    int make(gnn_mlp_group *g_, int iterations_, int validation_size_, size_t n_rows) {
        g = g_; validation_size = validation_size_; iterations = iterations_; stride = pad_up(validation_size);
        if (n_rows) TRY(rows.alloc(sizeof(float) * n_rows * (size_t)stride));
        TRY(val.alloc(sizeof(double) * (size_t)iterations * g->K));
        d_rows = rows.as<float>(); d_val = val.as<double>();
        return GNN_OK;
    }
    // (the loop has waited for the stream behind the last sum: one readback)  by_member: the sums lie [k][i], else [i][K]
    int read(bool by_member, double *val_loss) const {
        const int K = g->K;
        std::vector<double> sums((size_t)iterations * K);
        HIP_TRY(hipMemcpy(sums.data(), val.p, sizeof(double) * sums.size(), hipMemcpyDeviceToHost));
        for (size_t at = 0; at < sums.size(); at++) { // (at = i * K + k)
            const size_t i = at / K, k = at % K;
            val_loss[at] = sums[by_member ? k * iterations + i : at] / (double)validation_size; // NNT:112
        }
        return GNN_OK;
    }
};
struct GroupValidation : CurveObserver {
    int M;
    int summed = 0; // iterations whose rows are summed already (or whose sum is enqueued)
    int make(gnn_mlp_group *g_, int iterations_, int validation_size_) {
        M = std::min(iterations_, kCurveRows);
        return CurveObserver::make(g_, iterations_, validation_size_, (size_t)M * g_->K);
    }
    int sum_through(int i_end) {
        if (i_end == summed) return GNN_OK;
        TRY(enqueue_group_curve_sum(g, d_rows, i_end - summed, stride, validation_size, d_val + (size_t)summed * g->K)); // (summed is a multiple of M: matrix rows 0 ..)
        summed = i_end;
        return GNN_OK;
    }
    int after_step(int i) override {
        TRY(enqueue_group_validation(g, validation_size, d_rows + (size_t)(i % M) * g->K * stride, stride));
        return (i + 1) % M == 0 ? sum_through(i + 1) : GNN_OK;
    }
    int after_chunk(int i_end) override {
        TRY_LAUNCHES(g->m[0]);
        return i_end == iterations ? sum_through(i_end) : GNN_OK; // (in front of the loop's own wait for the stream)
    }
};
} // namespace

int gnn_mlp_group_observed_launches(const gnn_mlp_group_t *g) { return !g ? -1 : (g->grouped && g->K > 1 && g->eval_plan.ok) ? 3 : 0; }

int gnn_mlp_group_train_sampled_observed(gnn_mlp_group_t *g, gnn_sampler_t *s, int iterations, int batch, const double *steps,
                                         const double *momenta, int noise, int validation_size, double *val_loss) { return guarded([&]() -> int {
    TRY(check_group(g));
    TRY(check_per_member(g, steps, momenta));
    gnn_mlp *h0 = g->m[0];
    TRY(train_sampled_checks(h0, s, iterations, batch, steps[0], noise));
    if (!val_loss) return fail(GNN_ERR_BAD_ARG, "null output");
    if (validation_size <= 0 || validation_size > h0->dataset_n) return fail(GNN_ERR_BAD_ARG, "validation size outside the dataset (NNT:104)");
    if (gnn_mlp_group_observed_launches(g) != 3) // member after member, the sampler rewound for each
        return members_one_sampler(g, s, iterations, batch, steps, momenta, noise, validation_size, val_loss);
    GroupValidation obs;
    TRY(obs.make(g, iterations, validation_size));
    TRY(GroupedCall{g}.run(steps, momenta, [&](GroupLaunch &) { return train_sampled_run(h0, &s, 1, iterations, &batch, steps[0], momenta[0], noise, &obs, nullptr); }));
    return obs.read(false, val_loss);
}); }

} // extern "C"

/* One sampler per member.  The loop is train_sampled_run on member 0 with K index rings (sampler.hip); an iteration in
 * which every member's batch has the same size is the two grouped launches, member k reading ring k through the index region
 * (group_kernels.h).  A refill shortens a batch per member (NNT:149-155), so around a refill the sizes may differ: such a
 * MIXED iteration is stepped member after member through the members' own handles, outside the GroupScope -- the lone step by
 * construction.  Nothing is announced for it and every member's look-ahead state is forgotten on both sides of it (bitwise
 * neutral: one forward-only launch when the grouped chain resumes). */
namespace {
// What both forms of the group's side share: the index region's way into the launches' arguments and out of the members' states.
// sizes: the per-member sizes the members leave the region with (a sized call's), or null.
struct MemberRegion : SampledEach {
    gnn_mlp_group *g; GroupLaunch *gl; const GroupSizes *sizes;
    MemberRegion(gnn_mlp_group *g_, GroupLaunch *gl_, const GroupSizes *sizes_) : g(g_), gl(gl_), sizes(sizes_) {}
    ~MemberRegion() override { if (gl->idx_lo) MemberRegion::region(nullptr, 0); } // (the loop was left by an exception)
    void region(const int32_t *lo, size_t slice_bytes) override {
        if (!lo) { // about to be released: no member keeps an address inside it
            leave_grouped(g, 0, gl->idx_lo, gl->idx_S, sizes);
            for (gnn_mlp *h : g->m) h->la.index_region_released();
        }
        gl->idx_lo = reinterpret_cast<const char *>(lo); gl->idx_S = slice_bytes;
    }
};
struct EachMember : MemberRegion {
    const double *steps, *momenta;
    int64_t &mixed; // (the call's: GroupedCall::run hands the members the grouped iterations only)
    EachMember(GroupedCall &call, GroupLaunch &gl_, const double *steps_, const double *momenta_)
        : MemberRegion(call.g, &gl_, nullptr), steps(steps_), momenta(momenta_), mixed(call.mixed) {}
    void forget_all() { // member 0's state for everyone (one staging buffer index for all), then forgotten
        for (int k = 0; k < g->K; k++) { g->m[k]->la = g->m[0]->la.rebased(g->arena, g->S, k, gl->idx_lo, gl->idx_S); g->m[k]->la.forget(); }
    }
    int mixed_step(const int32_t *const *d_idx, const int *counts) override {
        gnn_mlp *h0 = g->m[0];
        h0->grp = nullptr; // (outside the GroupScope; set again below on every path)
        forget_all();
        int rc = GNN_OK;
        for (int k = 0; k < g->K && rc == GNN_OK; k++)
            rc = step_on_device_indices(g->m[k], d_idx[k], counts[k], steps[k], momenta[k]);
        forget_all();
        h0->grp = gl;
        mixed++;
        return rc;
    }
};
} // namespace

/* One batch size per member (the reference's recorded sweep, logs/trainLog.csv rows 1-3: three step sizes AND three batch sizes).
 * The loop is the one above with ring m drawn at batches[m]; EVERY iteration is the two grouped launches, member k with its own
 * live row count now and in the announced iteration (GroupLaunch::rows / next_rows, group_kernels.h) -- a refill that shortens
 * one member's batch changes that member's entry, nothing else.  The per-iteration decision is group_sizes.h's. */
namespace {
struct SizedMembers : MemberRegion {
    GroupSizes &track; // member k's sizes of the batches member 0's state names, step by step (the call's: the members leave with them)
    SizedMembers(GroupedCall &call, GroupLaunch &gl_) : MemberRegion(call.g, &gl_, &call.track), track(call.track) { track = g->sizes; }
    int mixed_step(const int32_t *const *, const int *) override { return fail(GNN_ERR_STATE, "a sized group call steps no iteration member after member"); }
    bool sized() const override { return true; }
    void step_sizes(const int *rows, const int *next_rows) override {
        const SizedStep s = make_sized_step(g->K, rows, next_rows);
        for (int k = 0; k < g->K; k++) { gl->rows[k] = s.rows[k]; gl->next_rows[k] = s.next_rows[k]; }
        gl->next_same_rows = s.next_same_rows;
        track.stepped(g->K, s);
    }
};
// The observed form of a sized call.  Column k is the lone handle's curve BIT FOR BIT, as the members are the lone nets: the
// grouped validation kernel (group_eval.hip) forms the per-row losses in another order than the single-net forward kernels and
// differs from them in the last bits (2e-7 relative on the curves of tests/test_group_batches_gpu.py), so behind every grouped
// step each member's validation pass is the lone one (sampler.hip), through its own handle on the group's stream -- the forward
// kernels read the weights the step has just written and touch neither slabs nor staged rows.  Sums to val[k][i]: the per-row
// losses kept in rows[k][i][..] and summed by one launch behind the loop when that fits 1 GiB, else summed per iteration (the
// same fp64 sum either way: eval_kernels.h).
struct MemberValidation : CurveObserver {
    int make(gnn_mlp_group *g_, int iterations_, int validation_size_) {
        const int K = g_->K;
        const bool rows_form = eval_block_rows(g_->m[0], validation_size_) >= validation_size_ && (int64_t)K * iterations_ * pad_up(validation_size_) * 4 <= (1ll << 30);
        return CurveObserver::make(g_, iterations_, validation_size_, rows_form ? (size_t)K * (size_t)iterations_ : 0);
    }
    int after_step(int i) override {
        for (int k = 0; k < g->K; k++) {
            gnn_mlp *h = g->m[(size_t)k];
            const size_t at = (size_t)k * iterations + i;
            int vrc = GNN_OK;
            if (d_rows && validation_losses_to_row(h, validation_size, d_rows + at * stride, &vrc)) { TRY(vrc); continue; }
            TRY(validation_loss_sum(h, validation_size, d_val + at));
        }
        return GNN_OK;
    }
    int after_chunk(int) override {
        for (gnn_mlp *h : g->m) TRY_LAUNCHES(h);
        return GNN_OK;
    }
};

// gnn_mlp_group_train_sampled_each (`sized` false: batches[] holds the one size K times) and gnn_mlp_group_train_sampled_sizes:
// one call, but for who stands on the group's side of the loop (EachMember / SizedMembers), who observes it (GroupValidation:
// sums [i][K] every kCurveRows iterations / MemberValidation: sums [k][i]) and what GroupedCall makes of a mixed iteration.
int train_sampled_members(gnn_mlp_group *g, gnn_sampler_t *const *samplers, int iterations, const int *batches, const double *steps,
                          const double *momenta, int noise, int validation_size, double *val_loss, bool sized) {
    TRY(check_group(g));
    TRY(check_per_member(g, steps, momenta));
    const int K = g->K;
    gnn_mlp *h0 = g->m[0];
    if (samplers && !batches) return fail(GNN_ERR_BAD_ARG, "batches is null: one batch size per member"); // (_sizes: _each has its own array)
    TRY(check_member_samplers(g, samplers, iterations, batches, steps, noise, validation_size, val_loss));
    g->each_grouped = g->each_mixed = 0;
    if (K == 1 || !g->grouped || (val_loss && gnn_mlp_group_observed_launches(g) != 3)) { // member after member
        TRY(members_own_samplers(g, samplers, iterations, batches, steps, momenta, noise, validation_size, val_loss));
        g->each_mixed = iterations;
        return GNN_OK;
    }
    GroupValidation together;
    MemberValidation alone;
    CurveObserver *obs = nullptr;
    if (val_loss && !sized) { TRY(together.make(g, iterations, validation_size)); obs = &together; }
    if (val_loss && sized) { TRY(alone.make(g, iterations, validation_size)); obs = &alone; }
    GroupedCall call{g, sized, /* counted */ true};
    TRY(call.run(steps, momenta, [&](GroupLaunch &gl) {
        auto loop = [&](SampledEach *each) { return train_sampled_run(h0, samplers, K, iterations, batches, steps[0], momenta[0], noise, obs, each); };
        if (sized) { SizedMembers each(call, gl); return loop(&each); }
        EachMember each(call, gl, steps, momenta);
        return loop(&each);
    }));
    if (!val_loss) return GNN_OK;
    if (sized && alone.d_rows) { // the per-row losses were kept: their sums in one launch
        hipLaunchKernelGGL(sum_rows_kernel, dim3((unsigned)K * (unsigned)iterations), dim3(256), 0, h0->stream,
                           RowSumParams{alone.d_rows, alone.stride, validation_size, alone.d_val});
        TRY_LAUNCHES(h0);
        HIP_TRY(hipStreamSynchronize(h0->stream));
    }
    return obs->read(sized, val_loss); // (val[k][i] of a sized call: transposed on the host)
}
} // namespace

extern "C" {

int gnn_mlp_group_train_sampled_each(gnn_mlp_group_t *g, gnn_sampler_t *const *samplers, int iterations, int batch,
                                     const double *steps, const double *momenta, int noise, int validation_size,
                                     double *val_loss) { return guarded([&]() -> int {
    int batches[GROUP_MAX];
    std::fill(batches, batches + GROUP_MAX, batch);
    return train_sampled_members(g, samplers, iterations, batches, steps, momenta, noise, validation_size, val_loss, false);
}); }

int gnn_mlp_group_train_sampled_sizes(gnn_mlp_group_t *g, gnn_sampler_t *const *samplers, int iterations, const int32_t *batches,
                                      const double *steps, const double *momenta, int noise, int validation_size,
                                      double *val_loss) { return guarded([&]() -> int {
    return train_sampled_members(g, samplers, iterations, batches, steps, momenta, noise, validation_size, val_loss, true);
}); }

} // extern "C"

/* The held-out curve of a group (include/gnn_mlp.h: gnn_mlp_group_train_sampled_held_out): the sized loop above with, behind the
 * iterations that end an interval and still under the GroupScope, the launches of gnn_mlp_group_evaluate_set_range over the
 * held-out rows -- their results left in slot p of a device buffer [P][K hit counters, the ensemble's, K loss sums] -- and ONE
 * keep_best launch for all members (keep_best_kernel.h).  Groups without grouped launches train interval by interval, member
 * after member through their own handles (a lone loop cut into calls ends on the same bits), the point behind every interval. */
namespace {
struct GroupHeldOut : SampledObserver {
    gnn_mlp_group *g; int iterations, every, rule, P; int64_t held_rows;
    unsigned long long *d_res; double *d_slots;
    bool want_weights;
    std::vector<unsigned long long> res; std::vector<KeepBestRecord> best; std::vector<float> w;
    size_t words() const { return 2 * (size_t)g->K + 1; }
    int point(int p) {
        unsigned long long *hits = d_res + (size_t)p * words();
        double *sums = reinterpret_cast<double *>(hits + (g->K + 1));
        TRY(enqueue_group_point(g, held_rows, hits, sums, d_slots));
        return launch_keep_best(g->m[0]->stream, g->m.data(), g->K, hits, sums, p, rule);
    }
    int readbacks() {
        hipStream_t st = g->m[0]->stream;
        HIP_TRY(hipMemcpyAsync(res.data(), d_res, sizeof(unsigned long long) * res.size(), hipMemcpyDeviceToHost, st));
        for (int k = 0; k < g->K; k++) {
            const gnn_mlp *h = g->m[(size_t)k];
            HIP_TRY(hipMemcpyAsync(&best[(size_t)k], h->best_hist + (P - 1), sizeof(KeepBestRecord), hipMemcpyDeviceToHost, st));
            if (want_weights) HIP_TRY(hipMemcpyAsync(w.data() + (size_t)k * h->n_pad, h->best_W, sizeof(float) * (size_t)h->n_pad, hipMemcpyDeviceToHost, st));
        }
        return GNN_OK;
    }
    int after_step(int i) override {
        if ((i + 1) % every != 0 && i + 1 != iterations) return GNN_OK;
        return point(i / every);
    }
    int after_chunk(int i_end) override {
        for (gnn_mlp *h : g->m) TRY_LAUNCHES(h);
        return i_end == iterations ? readbacks() : GNN_OK; // (in front of the loop's own wait for the stream)
    }
};
} // namespace

extern "C" {

int gnn_mlp_group_train_sampled_held_out(gnn_mlp_group_t *g, gnn_sampler_t *const *samplers, int iterations, const int32_t *batches,
                                         const double *steps, const double *momenta, int noise, int every, int64_t held_rows, int rule,
                                         int64_t *point_hits, double *point_loss, int64_t *ensemble_hits, int32_t *best_point,
                                         double *best_weights) { return guarded([&]() -> int {
    TRY(check_group(g));
    TRY(check_per_member(g, steps, momenta));
    const int K = g->K;
    gnn_mlp *h0 = g->m[0];
    if (samplers && !batches) return fail(GNN_ERR_BAD_ARG, "batches is null: one batch size per member");
    TRY(check_member_samplers(g, samplers, iterations, batches, steps, noise, 0, nullptr));
    TRY(check_held_out_args(h0, every, held_rows, rule, point_hits, point_loss, best_point));
    for (gnn_mlp *h : g->m) TRY(check_handle(h)); // (a member's deferred host-batch update is applied first)
    const int P = gnn_mlp_held_out_points(iterations, every);
    for (gnn_mlp *h : g->m) TRY(ensure_keep_best(h, P));
    TRY(prepare_group_point(g, held_rows));
    GroupHeldOut obs;
    obs.g = g; obs.iterations = iterations; obs.every = every; obs.rule = rule; obs.P = P; obs.held_rows = held_rows;
    const size_t res_b = sizeof(unsigned long long) * obs.words() * (size_t)P;
    const size_t need = res_b + sizeof(double) * (size_t)group_point_slots(g, held_rows);
    if (g->held_res_bytes < need) {
        HIP_TRY(hipStreamSynchronize(g->stream));
        if (g->held_res) (void)hipFree(g->held_res);
        g->held_res = nullptr; g->held_res_bytes = 0;
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&g->held_res), need));
        g->held_res_bytes = need;
    }
    HIP_TRY(hipMemsetAsync(g->held_res, 0, res_b, h0->stream));
    obs.d_res = reinterpret_cast<unsigned long long *>(g->held_res);
    obs.d_slots = reinterpret_cast<double *>(g->held_res + res_b);
    obs.want_weights = best_weights != nullptr;
    obs.res.assign(obs.words() * (size_t)P, 0);
    obs.best.assign((size_t)K, KeepBestRecord{0, 0.0, -1, 0});
    if (best_weights) obs.w.assign((size_t)K * (size_t)h0->n_pad, 0.f);
    g->each_grouped = g->each_mixed = 0;
    if (K == 1 || !g->grouped) { // interval by interval, member after member, each with its own sampler and batch size through its own handle
        for (int p = 0; p < P; p++) {
            const int n_it = std::min(every, iterations - p * every);
            TRY(members_own_samplers(g, samplers, n_it, batches, steps, momenta, noise));
            TRY(obs.point(p));
        }
        for (gnn_mlp *h : g->m) TRY_LAUNCHES(h);
        TRY(obs.readbacks());
        HIP_TRY(hipStreamSynchronize(h0->stream));
        g->each_mixed = iterations;
    } else {
        GroupedCall call{g, /* sized */ true, /* counted */ true};
        TRY(call.run(steps, momenta, [&](GroupLaunch &gl) {
            SizedMembers each(call, gl);
            return train_sampled_run(h0, samplers, K, iterations, batches, steps[0], momenta[0], noise, &obs, &each);
        }));
        // (the loop has waited for the stream behind the readbacks: the ONE synchronisation)
    }
    static_assert(sizeof(unsigned long long) == sizeof(double), "one buffer for counters and sums");
    for (int p = 0; p < P; p++) {
        const unsigned long long *row = obs.res.data() + (size_t)p * obs.words();
        for (int k = 0; k < K; k++) {
            point_hits[(size_t)p * K + k] = (int64_t)row[k];
            std::memcpy(&point_loss[(size_t)p * K + k], &row[K + 1 + k], sizeof(double));
        }
        if (ensemble_hits) ensemble_hits[p] = (int64_t)row[K];
    }
    for (int k = 0; k < K; k++) {
        best_point[k] = obs.best[(size_t)k].at;
        if (best_weights && best_point[k] >= 0) {
            const std::vector<float> wk(obs.w.begin() + (size_t)k * h0->n_pad, obs.w.begin() + (size_t)(k + 1) * h0->n_pad);
            unpack_params(h0, wk, best_weights + (size_t)k * h0->n_params);
        }
    }
    return GNN_OK;
}); }

int gnn_mlp_group_sampled_each_iterations(const gnn_mlp_group_t *g, int64_t *grouped, int64_t *member_after_member) {
    if (!g || !grouped || !member_after_member) return GNN_ERR_BAD_ARG;
    *grouped = g->each_grouped; *member_after_member = g->each_mixed;
    return GNN_OK;
}

} // extern "C"
