// distill.hip -- targets of resident rows (include/gnn_mlp.h): the expected rows of a resident set read back and rewritten in
// place (gnn_mlp_get_targets_range, gnn_mlp_set_targets_range, gnn_mlp_group_set_targets_range), a lone net's output rows over a
// range (gnn_mlp_propagate_set_range), and a teacher's outputs blended into a student's resident expected rows on the device
// (gnn_mlp_distill_range, gnn_mlp_group_distill_range; distill_kernel.h).
//
// Rewriting expected rows invalidates nothing the handle has prepared ahead: the look-ahead state (lookahead.h) describes
// first-layer sums and staged copies of INPUT rows only -- the tile kernel (tile_step_kernel.h) has no expected-row argument,
// and the row-block kernel's staged copy (RbParams::xcopy) is of A_0 rows; expected rows are read by the step that runs on
// them (launch_small.hip: bind_call), by address, when it runs.  So no Lookahead member is called here.
#include "handle.h"
#include "distill_kernel.h"

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

using namespace gnn;
using namespace gnn::host;

namespace {

// the expected rows of set `set`, writable
float *target_rows(gnn_mlp *h, int set) { return set == GNN_SET_HELD_OUT ? h->held.Y : h->DY; }

// Y (fp64, [n][d_out]) -> rows [first, first + n) of the set's expected rows, converted as upload_dataset_f64 converts its Y
// (launch_convert_rows, no activation) through the handle's own export staging buffer in chunks of max_batch rows: no
// allocation.  Everything is enqueued on the handle's stream, behind what is in flight there.
int write_targets(gnn_mlp *h, int set, int64_t first, int64_t n, const double *Y) {
    const int Lm = h->L - 1, dl = h->dims[Lm], ldo = h->ld[Lm];
    float *dst = target_rows(h, set) + (size_t)first * ldo;
    const int64_t chunk = h->max_batch; // (stage_out holds max_batch x d_out doubles)
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int64_t rows = std::min<int64_t>(chunk, n - r0);
        HIP_TRY(hipMemcpyAsync(h->stage_out, Y + r0 * dl, sizeof(double) * (size_t)rows * dl, hipMemcpyHostToDevice, h->stream));
        launch_convert_rows(h, h->stage_out, dl, dst + (size_t)r0 * ldo, ldo, rows, rows, 0, 0);
        HIP_TRY(hipStreamSynchronize(h->stream)); // the staging buffer is reused by the next chunk
    }
    TRY_LAUNCHES(h);
    return GNN_OK;
}

// While a teacher runs on a student's rows its handle names them as its own training set: the bf16 forward pass finds the bf16
// twin of an input row through the handle's set (plan.hip: a0_bf16).  Nothing else reads the fields during a forward pass.
struct BorrowedSet {
    gnn_mlp *h; float *X, *Y; __bf16 *Xb; int64_t n;
    BorrowedSet(gnn_mlp *h_, const ResidentSet &rs) : h(h_), X(h_->DX), Y(h_->DY), Xb(h_->DXb), n(h_->dataset_n) {
        h->DX = rs.X; h->DY = rs.Y; h->DXb = rs.Xb; h->dataset_n = rs.n;
    }
    ~BorrowedSet() { h->DX = X; h->DY = Y; h->DXb = Xb; h->dataset_n = n; }
    BorrowedSet(const BorrowedSet &) = delete;
    BorrowedSet &operator=(const BorrowedSet &) = delete;
};

// gnn_mlp_evaluate_set_range's block loop (abi.hip: enqueue_evaluation) with the output rows kept: every block's padded rows
// gathered into dense[n][d_out], and -- blend_y: row `first` of the expected rows -- blended into them.  Enqueued only.
int enqueue_outputs(gnn_mlp *h, const ResidentSet &rs, int64_t first, int64_t n, float *dense, float *blend_y, float keep) {
    const int Lm = h->L - 1, d_out = h->dims[Lm], ldo = h->ld[Lm];
    const int block = eval_block_rows(h, n);
    int rc_ws = GNN_OK;
    EvalScope scope(h, block, &rc_ws);
    if (rc_ws != GNN_OK) return rc_ws;
    for (int64_t off = 0; off < n; off += block) {
        const int B = (int)std::min<int64_t>(block, n - off);
        const float *y = rs.Y + (size_t)(first + off) * ldo;
        do_forward(h, rs.X + (size_t)(first + off) * h->ld[0], y, B, true, true, true);
        float *t = dense + (size_t)off * d_out;
        HIP_TRY(launch_gather_dense(h->prob, ldo, d_out, B, t, h->stream));
        if (blend_y) HIP_TRY(launch_blend(BlendParams{t, blend_y + (size_t)off * ldo, ldo, d_out, B, keep}, h->stream));
    }
    TRY_LAUNCHES(h);
    return GNN_OK;
}

// what both distillation calls refuse about the student, the rows and keep -- before any work
int check_student(const gnn_mlp *s, int64_t first, int64_t n, double keep) {
    if (!(keep >= 0.0 && keep <= 1.0)) return fail(GNN_ERR_BAD_ARG, "keep must lie in [0, 1]");
    if (s->group) return fail(GNN_ERR_STATE, "the student is a member of a group: its expected rows are the group's one copy, which every member trains on");
    if (s->dp_replica) return fail(GNN_ERR_STATE, "the student is a replica of a data-parallel handle: every replica holds its own copy of the rows");
    return check_set_rows(s, GNN_SET_TRAIN, first, n);
}
// ... and about the pair: the teacher must read the student's input rows as its own and write rows of the student's width
int check_pair(const gnn_mlp *s, const gnn_mlp *t) {
    const char *what = nullptr;
    if (t->dims[0] != s->dims[0] || t->ld[0] != s->ld[0]) what = "the input width (dims[0])";
    else if (t->dims[t->L - 1] != s->dims[s->L - 1] || t->ld[t->L - 1] != s->ld[s->L - 1]) what = "the output width (dims[L-1])";
    else if (t->inner_act != s->inner_act) what = "the inner activation (resident input rows hold f(x))";
    else if (t->dtype != s->dtype) what = "the dtype";
    else if (t->device != s->device) what = "the device";
    if (what) return fail(GNN_ERR_BAD_ARG, std::string("teacher and student differ in ") + what);
    return GNN_OK;
}

} // namespace

extern "C" {

int gnn_mlp_get_targets_range(gnn_mlp_t *h, int set, int64_t first, int64_t n, double *Y) { return guarded([&]() -> int {
    if (!h || !Y) return fail(GNN_ERR_BAD_ARG, "null argument");
    TRY(check_set_rows(h, set, first, n));
    TRY(check_handle(h));
    const int Lm = h->L - 1, dl = h->dims[Lm], ldo = h->ld[Lm];
    std::vector<float> tmp((size_t)n * dl);
    HIP_TRY(hipMemcpy2DAsync(tmp.data(), sizeof(float) * (size_t)dl, target_rows(h, set) + (size_t)first * ldo, sizeof(float) * (size_t)ldo,
                             sizeof(float) * (size_t)dl, (size_t)n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < tmp.size(); i++) Y[i] = (double)tmp[i];
    return GNN_OK;
}); }

int gnn_mlp_set_targets_range(gnn_mlp_t *h, int set, int64_t first, int64_t n, const double *Y) { return guarded([&]() -> int {
    if (!h || !Y) return fail(GNN_ERR_BAD_ARG, "null argument");
    if (set != GNN_SET_TRAIN && set != GNN_SET_HELD_OUT) return fail(GNN_ERR_BAD_ARG, "set: GNN_SET_TRAIN or GNN_SET_HELD_OUT");
    if (h->group) return fail(GNN_ERR_STATE, member_set_message(set));
    TRY(check_set_rows(h, set, first, n));
    TRY(check_handle(h)); // (a deferred host-batch update is applied first)
    return write_targets(h, set, first, n, Y);
}); }

int gnn_mlp_group_set_targets_range(gnn_mlp_group_t *g, int set, int64_t first, int64_t n, const double *Y) { return guarded([&]() -> int {
    if (!g || !Y) return fail(GNN_ERR_BAD_ARG, "null argument");
    TRY(check_set_rows(g->m[0], set, first, n));
    for (gnn_mlp *h : g->m) TRY(check_handle(h));
    return write_targets(g->m[0], set, first, n, Y); // (the one copy; members and group share one stream)
}); }

int gnn_mlp_propagate_set_range(gnn_mlp_t *h, int set, int64_t first, int64_t n, double *out) { return guarded([&]() -> int {
    if (!h || !out) return fail(GNN_ERR_BAD_ARG, "null argument");
    TRY(check_set_rows(h, set, first, n));
    TRY(check_handle(h));
    const int d_out = h->dims[h->L - 1];
    DevScratch dense;
    TRY(dense.alloc(sizeof(float) * (size_t)n * d_out));
    const int rc = enqueue_outputs(h, resident_set(h, set), first, n, dense.as<float>(), nullptr, 0.f);
    std::vector<float> tmp((size_t)n * d_out);
    hipError_t e = hipSuccess;
    if (rc == GNN_OK) e = hipMemcpyAsync(tmp.data(), dense.p, sizeof(float) * tmp.size(), hipMemcpyDeviceToHost, h->stream);
    const hipError_t es = hipStreamSynchronize(h->stream); // (also on failure: the scratch is released when this function returns)
    if (rc != GNN_OK) return rc;
    if (e != hipSuccess || es != hipSuccess) return fail(GNN_ERR_HIP, std::string("output readback: ") + hipGetErrorString(e != hipSuccess ? e : es));
    for (size_t i = 0; i < tmp.size(); i++) out[i] = (double)tmp[i];
    return GNN_OK;
}); }

int gnn_mlp_distill_range(gnn_mlp_t *student, gnn_mlp_t *teacher, int64_t first, int64_t n, double keep) { return guarded([&]() -> int {
    if (!student || !teacher) return fail(GNN_ERR_BAD_ARG, "null handle");
    TRY(check_student(student, first, n, keep));
    TRY(check_pair(student, teacher));
    TRY(check_handle(student));
    TRY(check_handle(teacher)); // (the teacher's deferred host-batch update is applied first)
    const float keep_f = (float)keep;
    if (keep_f == 1.f) return GNN_OK; // every bit of the rows stays
    const ResidentSet rs = resident_set(student, GNN_SET_TRAIN);
    const int d_out = student->dims[student->L - 1];
    HIP_TRY(hipStreamSynchronize(student->stream)); // nothing of the student's in flight still reads or writes the rows
    DevScratch dense;
    TRY(dense.alloc(sizeof(float) * (size_t)n * d_out));
    int rc;
    {
        BorrowedSet borrowed(teacher, rs);
        rc = enqueue_outputs(teacher, rs, first, n, dense.as<float>(), rs.Y + (size_t)first * student->ld[student->L - 1], keep_f);
    }
    const hipError_t es = hipStreamSynchronize(teacher->stream);
    if (rc != GNN_OK) return rc;
    if (es != hipSuccess) return fail(GNN_ERR_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(es));
    return GNN_OK;
}); }

int gnn_mlp_group_distill_range(gnn_mlp_t *student, gnn_mlp_group_t *teachers, int64_t first, int64_t n, double keep) { return guarded([&]() -> int {
    if (!student || !teachers) return fail(GNN_ERR_BAD_ARG, "null handle");
    TRY(check_student(student, first, n, keep));
    TRY(check_pair(student, teachers->m[0]));
    TRY(check_handle(student));
    for (gnn_mlp *h : teachers->m) TRY(check_handle(h)); // (each teacher's deferred host-batch update is applied first)
    const float keep_f = (float)keep;
    if (keep_f == 1.f) return GNN_OK; // every bit of the rows stays
    const ResidentSet rs = resident_set(student, GNN_SET_TRAIN);
    HIP_TRY(hipStreamSynchronize(student->stream)); // nothing of the student's in flight still reads or writes the rows
    std::vector<std::unique_ptr<BorrowedSet>> borrowed; // (the member-after-member form runs every member's own forward pass)
    for (gnn_mlp *h : teachers->m) borrowed.emplace_back(new BorrowedSet(h, rs));
    return group_distill_rows(teachers, rs, first, n, rs.Y + (size_t)first * student->ld[student->L - 1], keep_f);
}); }

} // extern "C"
