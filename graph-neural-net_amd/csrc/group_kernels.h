// group_kernels.h -- the two-launch step (rowblock_kernel.h, tile_step_kernel.h) for a GROUP of nets of one shape: one launch
// serves every member, blockIdx.y = the member.
//
// The pointer rule.  Every per-member device buffer a training launch touches is carved out of one arena, member k's slice
// at member 0's + k * S (group.hip), so a grouped launch takes member 0's parameters exactly as the single-net host code
// builds them and member k turns each pointer p into p + k * S when (p - arena_lo) < S (unsigned), and leaves it alone
// otherwise: what all members share -- the group's data set, the device index ring of a call with one shared sampler --
// lies outside the arena.  Null stays null.  The arithmetic is the single-net kernels' (the same bodies), run at a different
// blockIdx.
//
// The index region.  A call with one sampler per member (gnn_mlp_group_train_sampled_each) keeps K device index rings in one
// allocation outside the arena, member 0's in [idx_lo, idx_lo + idx_S), member k's the same layout at + k * idx_S.  For the
// INDEX pointers only (row_idx, copy_idx, next_idx) a pointer inside member 0's ring moves by k * idx_S; any other index
// pointer (a member's idxbuf lies in the arena) follows the arena rule.  idx_S == 0 -- every other call -- matches nothing.
//
// The row counts.  In every call but one all members step batches of ONE size: the row counts are member 0's, the scalars of the
// single-net arguments.  A call with one batch size per member (gnn_mlp_group_train_sampled_sizes) launches the SIZED twins, which
// take one more argument, GroupRows: rows[k] live rows in member k's batch being stepped, next_rows[k] in its announced next
// one; the padded counts are pad_up of these.  Member k's buffers are read and written over pad_up(rows[k]) rows exactly as
// the lone net's are -- rows >= rows[k] are zeros up to the pad -- and everything a kernel decides from a row
// count is decided from blockIdx.y's, so it stays block-uniform: one launch holds workgroups on the full-chunk paths (a
// member with 128 rows or more) beside workgroups on the guarded ones, and members of one and of two TS_KC chunks.  Twins, not
// one kernel with equal entries: with the counts read from an array the uniform step measured 0.2-1.3 % slower at K = 8 / 16
// and 3-4 % at K = 2 on the small net, outside the parent's run-to-run spread.
#pragma once
#include "rowblock_kernel.h"
#include "tile_step_kernel.h"

namespace gnn {

constexpr int GROUP_MAX = 16; // members of one group (include/gnn_mlp.h: gnn_mlp_group_create)

struct GroupArgs {
    const char *arena_lo;         // member 0's slice of the arena
    unsigned long long S;         // bytes per member
    const char *idx_lo;           // member 0's slice of the index region (below); beside arena_lo / S: one cache line, one load
    unsigned long long idx_S;     // bytes per member; 0: no region
    int nbx;                      // live workgroups per member along x (the grid is padded to a multiple of 8: XCD placement)
    float step_over_b[GROUP_MAX]; // (float)(step_k / (double)B), as step_on_rows computes it -- B: member k's own in a sized launch
    float momentum[GROUP_MAX];
};
// the last argument of the sized twins
struct GroupRows {
    int rows[GROUP_MAX];      // live rows of member k's current batch ...
    int next_rows[GROUP_MAX]; // ... and of its next batch (tile kernels with FWD; a forward-only launch: the batch itself)
};

// member k's copy of a pointer of member 0 (the pointer rule above)
template <class T> __device__ __forceinline__ T *group_rel(T *q, const GroupArgs &g, unsigned long long shift) {
    const unsigned long long d = (unsigned long long)reinterpret_cast<const char *>(q) - (unsigned long long)g.arena_lo;
    return d < g.S ? reinterpret_cast<T *>((unsigned long long)q + shift) : q;
}
// ... of an index pointer: the index region first, else the arena rule (wave-uniform scalar arithmetic on kernel arguments)
__device__ __forceinline__ const int32_t *group_rel_idx(const int32_t *q, const GroupArgs &g, unsigned long long shift) {
    const unsigned long long a = (unsigned long long)reinterpret_cast<const char *>(q);
    // (masks, not selects: the row-block kernel's first index load waits for this)
    const unsigned long long in_idx = 0ull - (unsigned long long)(a - (unsigned long long)g.idx_lo < g.idx_S);
    const unsigned long long in_arena = 0ull - (unsigned long long)(a - (unsigned long long)g.arena_lo < g.S);
    return reinterpret_cast<const int32_t *>(a + ((in_idx & ((unsigned long long)blockIdx.y * g.idx_S)) | (~in_idx & in_arena & shift)));
}
// The tile bodies relocate a pointer at each use, inside their loops, and their two index pointers are p.row_idx and
// p.next_idx: both are relocated ONCE at the kernel's top (GroupIdx), and a use picks its copy by comparing addresses -- equal
// addresses have equal copies, so the choice is exact whichever of the two fields the body names.
struct GroupIdx { const int32_t *row0, *row, *next; };
template <class T> __device__ __forceinline__ T *group_rel(T *q, const GroupArgs &g, unsigned long long shift, const GroupIdx &) { return group_rel(q, g, shift); }
__device__ __forceinline__ const int32_t *group_rel(const int32_t *q, const GroupArgs &, unsigned long long, const GroupIdx &ix) { return q == ix.row0 ? ix.row : ix.next; }

// the tile kernel bodies (tile_step_body.inc) for member blockIdx.y: its pointers, its step and momentum; the row counts are
// member 0's (the plain fields) or, in the sized twins, its own
// (TS_HEAD_PROLOGUE 0, TS_DEFER_WV 0: the struct-only, lookup-only prologue with W and V requested at the top -- the grouped
// twins have no head arguments, tile_step_kernel.h, and compile to the code they had before the single-net kernels got theirs)
#define TS_HEAD_PROLOGUE 0
#define TS_DEFER_WV 0
#define TS_MERGE_KINDS 0 // (the merged map's workgroup kinds: single-net f32 only)
#define TS_HAS_ROW_IDX TS_REL(p.row_idx)
#define TS_STAGE_N L.N
#define TS_BID blockIdx.x
#define TS_REL(q) group_rel((q), ga, ga_shift, ga_idx)
#define TS_REL_LAYER(L) (L.A = TS_REL(L.A), L.D = TS_REL(L.D), L.W = TS_REL(L.W), L.V = TS_REL(L.V), L.G = TS_REL(L.G))
#define TS_STEP_OVER_B ga.step_over_b[blockIdx.y]
#define TS_MOMENTUM ga.momentum[blockIdx.y]
#define TS_K p.K
#define TS_K_TRUE p.k_true
#define TS_NEXT_ROWS p.next_rows
#define TS_NEXT_K p.next_K
template <int GSRC, int GDST, bool FWD>
__global__ __launch_bounds__(TS_THREADS) void tile_step_group_kernel(TileStepParams p, GroupArgs ga) {
    static_assert(GSRC <= 2, "grouped tile kernels: single-GPU forms only");
    const unsigned long long ga_shift = (unsigned long long)blockIdx.y * ga.S;
    const GroupIdx ga_idx{p.row_idx, group_rel_idx(p.row_idx, ga, ga_shift), group_rel_idx(p.next_idx, ga, ga_shift)};
#include "tile_step_body.inc"
}
template <int GSRC, int GDST, bool FWD>
__global__ __launch_bounds__(TS_THREADS) void tile_step_bf16_group_kernel(TileStepParams p, GroupArgs ga) {
    static_assert(GSRC <= 2, "grouped tile kernels: single-GPU forms only");
    const unsigned long long ga_shift = (unsigned long long)blockIdx.y * ga.S;
    const GroupIdx ga_idx{p.row_idx, group_rel_idx(p.row_idx, ga, ga_shift), group_rel_idx(p.next_idx, ga, ga_shift)};
#include "tile_step_bf16_body.inc"
}
#undef TS_K
#undef TS_K_TRUE
#undef TS_NEXT_ROWS
#undef TS_NEXT_K
// the sized twins: the four row counts are member blockIdx.y's (scalar loads from the kernel arguments at a block-uniform index,
// once at the top; every test on them in the bodies is block-uniform as it was)
#define TS_K ga_K
#define TS_K_TRUE ga_k_true
#define TS_NEXT_ROWS ga_next_rows
#define TS_NEXT_K ga_next_K
#define GNN_GROUP_ROW_COUNTS                                                                      \
    const int ga_k_true = gr.rows[blockIdx.y], ga_K = pad_up(ga_k_true);                          \
    const int ga_next_rows = gr.next_rows[blockIdx.y], ga_next_K = pad_up(ga_next_rows);          \
    (void)ga_k_true; (void)ga_K; (void)ga_next_rows; (void)ga_next_K;
template <int GSRC, int GDST, bool FWD>
__global__ __launch_bounds__(TS_THREADS) void tile_step_group_sized_kernel(TileStepParams p, GroupArgs ga, GroupRows gr) {
    static_assert(GSRC <= 2, "grouped tile kernels: single-GPU forms only");
    const unsigned long long ga_shift = (unsigned long long)blockIdx.y * ga.S;
    const GroupIdx ga_idx{p.row_idx, group_rel_idx(p.row_idx, ga, ga_shift), group_rel_idx(p.next_idx, ga, ga_shift)};
    GNN_GROUP_ROW_COUNTS
#include "tile_step_body.inc"
}
template <int GSRC, int GDST, bool FWD>
__global__ __launch_bounds__(TS_THREADS) void tile_step_bf16_group_sized_kernel(TileStepParams p, GroupArgs ga, GroupRows gr) {
    static_assert(GSRC <= 2, "grouped tile kernels: single-GPU forms only");
    const unsigned long long ga_shift = (unsigned long long)blockIdx.y * ga.S;
    const GroupIdx ga_idx{p.row_idx, group_rel_idx(p.row_idx, ga, ga_shift), group_rel_idx(p.next_idx, ga, ga_shift)};
    GNN_GROUP_ROW_COUNTS
#include "tile_step_bf16_body.inc"
}
#undef TS_HEAD_PROLOGUE
#undef TS_DEFER_WV
#undef TS_MERGE_KINDS
#undef TS_HAS_ROW_IDX
#undef TS_STAGE_N
#undef TS_BID
#undef TS_REL
#undef TS_REL_LAYER
#undef TS_STEP_OVER_B
#undef TS_MOMENTUM
#undef TS_K
#undef TS_K_TRUE
#undef TS_NEXT_ROWS
#undef TS_NEXT_K
#undef GNN_GROUP_ROW_COUNTS

// rowblock_kernel for member blockIdx.y: the head arguments and every pointer of the struct follow the pointer rule.  The text
// both kernels below run (a macro, not a function they call: the uniform kernel stays the instruction stream it was); ROWS: the
// member's live rows
#define GNN_RB_GROUP_MEMBER(ROWS)                                                                                                  \
    const unsigned long long sh = (unsigned long long)blockIdx.y * g.S;                                                            \
    p.slabs = group_rel(slabs, g, sh); p.row_idx = group_rel_idx(row_idx, g, sh); p.copy_idx = group_rel_idx(copy_idx, g, sh);     \
    _Pragma("unroll")                                                                                                              \
    for (int l = 0; l < MAX_LAYERS; l++) {                                                                                         \
        p.W[l] = group_rel(p.W[l], g, sh); p.act[l] = group_rel(p.act[l], g, sh); p.delta[l] = group_rel(p.delta[l], g, sh);       \
        p.Wb[l] = group_rel(p.Wb[l], g, sh); p.actb[l] = group_rel(p.actb[l], g, sh); p.deltab[l] = group_rel(p.deltab[l], g, sh); \
    }                                                                                                                              \
    p.prob = group_rel(p.prob, g, sh); p.loss = group_rel(p.loss, g, sh); p.label = group_rel(p.label, g, sh);                     \
    p.xcopy = group_rel(p.xcopy, g, sh); p.xcopyb = group_rel(p.xcopyb, g, sh);                                                    \
    p.X = group_rel(p.X, g, sh); p.Xb = group_rel(p.Xb, g, sh);                                                                    \
    if constexpr (BF) {                                                                                                            \
        p.Wb[1] = group_rel(reinterpret_cast<const __bf16 *>(W1), g, sh);                                                          \
        if constexpr (SH::kL > 0) p.Wb[SH::kL - 2] = group_rel(reinterpret_cast<const __bf16 *>(Wlast), g, sh);                    \
    } else {                                                                                                                       \
        p.W[1] = group_rel(W1, g, sh);                                                                                             \
        if constexpr (SH::kL > 0) p.W[SH::kL - 2] = group_rel(Wlast, g, sh);                                                       \
    }                                                                                                                              \
    p.Y = group_rel(Y, g, sh); p.B = (ROWS); p.slab_rows = slab_rows; p.ldy = ldy;                                                 \
    if constexpr (SH::is_static) {                                                                                                 \
        constexpr RbPlan m = SH::make();                                                                                           \
        static_assert(m.ok, "this shape does not fit the row-block kernel");                                                       \
        rowblock_body<SH::kL, true, ACT, OUTK, m.ns, (SH::kL >= 4 ? m.upw[1] : 0), BF>(m, p, blockIdx.x);                          \
    } else {                                                                                                                       \
        rowblock_body<SH::kL, false, ACT, OUTK, MID4_MAX_SLABS, (SH::kL == 3 ? 0 : RB_MAXU), BF>(p.plan, p, blockIdx.x);           \
    }
template <class SH, int ACT, int OUTK, bool BF = false>
__global__ __launch_bounds__(RB_NT) void rowblock_group_kernel(GNN_RB_HEAD_PARAMS, RbParams p, GroupArgs g) {
    static_assert(!BF || SH::kL == 3 || SH::kL == 4, "the bf16 row-block kernel: nets of three and four layers");
    if ((int)blockIdx.x >= g.nbx) return;
    GNN_RB_GROUP_MEMBER(B)
}
// the sized twin: the member's own row count (the head argument B is member 0's and unused), and its own
// pad_up(rows) / 4 row blocks -- the grid is the largest member's, padded to a multiple of 8 (g.nbx: that member's blocks)
template <class SH, int ACT, int OUTK, bool BF = false>
__global__ __launch_bounds__(RB_NT) void rowblock_group_sized_kernel(GNN_RB_HEAD_PARAMS, RbParams p, GroupArgs g, GroupRows gr) {
    static_assert(!BF || SH::kL == 3 || SH::kL == 4, "the bf16 row-block kernel: nets of three and four layers");
    const int rows = gr.rows[blockIdx.y];
    (void)B;
    if ((int)blockIdx.x >= pad_up(rows) / 4) return;
    GNN_RB_GROUP_MEMBER(rows)
}
#undef GNN_RB_GROUP_MEMBER

} // namespace gnn
