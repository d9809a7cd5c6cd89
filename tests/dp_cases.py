"""Who shards what: the data-parallel cases that tests/test_dp_shapes_gpu.py runs on gnn_mlp_dp_* handles, and Python
restatements of the host rules those handles apply (tests/test_dp_cases_cpu.py pins both; no GPU needed).

A case is one of the 24 drawn nets of tests/chain_cases.py with a replica count from the table REPLICAS below, or one of
the hand-picked EXTRAS.  Nothing here is random at test time: the table is written down, and the conditions it has to
meet (every replica count 1..16 that matters, replicas without rows, one-row shards, shards ragged against the 4-row blocks,
slice boundaries inside a layer's matrix, short and empty last slices) are asserted by the CPU test.

The host rules (csrc/dp.hip):
  shard(B, r, n)         dp_shard: contiguous row blocks, the first B % n replicas get one more row
  slice_floats(n_pad, n) gnn_mlp_dp_create: floats per owner of GNN_REDUCE_DIRECT_RS, ceil(ceil(n_pad / n) / 16) * 16
  n_pad(dims)            gnn_mlp_create: sum over layers of pad16(d_l) * pad16(d_{l+1}), the flat gradient buffer"""
import numpy as np

from tests import chain_cases as cc

DP_MAX_REPLICAS = 16

# Replicas of drawn case `seed` (its batch size in the comment).  16 goes to three of the nets whose batch is smaller than 16
# (replicas without rows); 8 to a batch that leaves its last replica ONE row (seed 15) and to two GeneralNeuralNets; seed 9 stays
# a handle of one replica; seed 7 (input width 1025, off the two-launch path) and the 1023 / 1024 edges are sharded.
REPLICAS = [16, 4, 3, 16, 5, 8, 7, 2,      # B = 15 13 50 11 24 62 19 42
            4, 1, 3, 8, 16, 7, 5, 8,       # B = 26 27 41 48 12 55 38 15
            2, 3, 4, 5, 2, 7, 3, 4]        # B = 34 44 37 21 46 21 38 53

# (dims, B, inner_act, out_kind, last_act, replicas): cases no draw gives
EXTRAS = [
    # two layers (per-layer GEMMs, step_launches == 0); n_pad = 256, slice = 48: owners 0..4 hold 48 floats, owner 5 holds 16,
    # owner 6 none (its reduce-scatter launch is skipped); shards 2 2 1 1 1 1 1
    ([1, 2], 9, 0, cc.OUT_SOFTMAX_CE, 4, 7),
    # a tiny three-layer GeneralNeuralNet (tanh inside, identity last) on 16 replicas with 3 rows: 13 replicas have none
    ([3, 5, 2], 3, 2, cc.OUT_ACT_LOSS, 4, 16),
    # 16 replicas that ALL have rows (shards 2 1 1 ... 1): the 16th term of every rank-ordered sum is a real partial gradient,
    # on a small four-layer net that takes the two-launch step (the fused GSRC = 3 / 4 sums as well as the flat kernels)
    ([20, 12, 9, 4], 17, 1, cc.OUT_SOFTMAX_CE, 4, 16),
]
N_DRAWN = cc.N_CASES
N_DP_CASES = N_DRAWN + len(EXTRAS)
CASE_IDS = ["s%d" % s for s in range(N_DRAWN)] + ["x%d" % i for i in range(len(EXTRAS))]

# Steps of the walk every case takes (see walk_calls()).  RANGE_CALLS: (first batch, steps) of the train_range calls on whole
# batches over the five resident batches -- the first and the third wrap, the state after the first is
# "after 3 steps", after the second "after 5 steps" (the bf16 oracle's checkpoints).
RANGE_CALLS = ((4, 3), (2, 2), (4, 4))
LONG_RANGE_CALL = (0, 6)      # the cases of LONG_CASES go on: past every replica's 16th gradient computation (hiprtc instantiation)
LONG_CASES = (7, 10, 16, 20)  # two or three replicas each (the instantiation pause is per replica); seed 7 is off the two-launch path


def dp_case(i):
    """dims, B, inner_act, out_kind, last_act, replicas, data seed of case i (0..23 drawn, then the extras)."""
    if i < N_DRAWN:
        dims, B, inner, out_kind, last = cc.chain_case(i)
        return dims, B, inner, out_kind, last, REPLICAS[i], i
    dims, B, inner, out_kind, last, n = EXTRAS[i - N_DRAWN]
    return list(dims), B, inner, out_kind, last, n, 100 + i


def pad16(d):
    return (d + 15) // 16 * 16


def shard(B, r, n):
    """Rows [lo, hi) of the batch that replica r of n takes."""
    base, extra = divmod(B, n)
    lo = r * base + min(r, extra)
    return lo, lo + base + (1 if r < extra else 0)


def shard_sizes(B, n):
    return [hi - lo for lo, hi in (shard(B, r, n) for r in range(n))]


def layer_offsets(dims):
    """Offset of every layer's padded matrix in the flat buffer, and the buffer's length n_pad."""
    offs, off = [], 0
    for a, b in zip(dims[:-1], dims[1:]):
        offs.append(off)
        off += pad16(a) * pad16(b)
    return offs, off


def n_pad(dims):
    return layer_offsets(dims)[1]


def slice_floats(n_pad_, n):
    return (((n_pad_ + n - 1) // n) + 15) // 16 * 16


def owner_range(n_pad_, n, r):
    """Floats [lo, hi) of the flat buffer that owner r reduces under GNN_REDUCE_DIRECT_RS (empty when lo == hi)."""
    s = slice_floats(n_pad_, n)
    return min(r * s, n_pad_), min((r + 1) * s, n_pad_)


def padded_index(dims):
    """For every weight of the unpadded flat vector (get_weights order) its offset in the padded flat buffer."""
    offs, _ = layer_offsets(dims)
    out = []
    for off, a, b in zip(offs, dims[:-1], dims[1:]):
        out.append((off + np.arange(a)[:, None] * pad16(b) + np.arange(b)[None, :]).ravel())
    return np.concatenate(out)


def short_rows(B, n):
    """Rows of the two kinds of short batch that end the walk: fewer than the replicas, so that replicas which had rows in
    the step of the same parity before (their gradient buffer holds that partial gradient) now have none; the second is
    shorter again."""
    b = max(1, min(B, n) - 1) if n > 1 else max(1, B // 2)
    return b, max(1, b // 2)


def walk_calls(B, n, long_case=False):
    """The calls a data-parallel handle of n replicas takes: ('train', first row, rows, steps) = train_range, ('step', first
    row, rows) = gradient_step_range at rows that are no multiple of B, ('host', first row, rows) = gradientStep on the host
    copy of resident rows.  The batch is B rows (constant shards) until the short tail: two train_range steps -- one per
    parity of the gradient buffers -- and one host batch with fewer rows than replicas.  The oracle budgets apply to the
    steps before the tail; the tail is held by the bitwise checks (why: tests/test_dp_cases_cpu.py,
    test_a_batch_of_a_few_rows_is_outside_the_oracle_budget)."""
    N = cc.dataset_rows(B)
    b, b2 = short_rows(B, n)
    calls = [("train", first * B, B, k) for first, k in RANGE_CALLS]
    calls += [("step", 1, B), ("step", N - B, B), ("host", B // 2, B)]
    if long_case:
        calls += [("train", LONG_RANGE_CALL[0] * B, B, LONG_RANGE_CALL[1]), ("step", (N - B) // 2, B)]
    calls += [("train", (N // b - 1) * b, b, 2), ("host", 2, b2)]
    return calls


TAIL_CALLS, TAIL_STEPS = 2, 3   # the short tail of walk_calls / walk


def walk(B, n, long_case=False):
    """The steps of walk_calls one by one, as (kind, first row, rows) with kind 'range' (a step of a train_range call: the
    handle announces its successor), 'step' or 'host'.  15 steps; 22 for a long case."""
    N = cc.dataset_rows(B)
    steps = []
    for call in walk_calls(B, n, long_case):
        if call[0] == "train":
            steps += [("range", r, call[2]) for r in cc.range_batches(N, call[2], call[1], call[3])]
        else:
            steps.append(call)
    assert all(0 <= f and 1 <= rows <= B and f + rows <= N for _, f, rows in steps)
    return steps


def case_data(i):
    dims, B, _, _, _, _, data_seed = dp_case(i)
    return cc.chain_data(data_seed, dims, B)


def case_oracle(oracle_mod, i):
    """The case's net in the fp64 C oracle with its start weights (the Random(1) draw, rounded to f32, times W_SCALE)."""
    dims, B, inner, out_kind, last, n, _ = dp_case(i)
    ref = oracle_mod.OracleNet(dims, out_kind=out_kind, inner_act=inner, last_act=last)
    ref.set_alloc_per_sample(0)
    w0 = ref.get_weights().astype(np.float32).astype(np.float64) * cc.W_SCALE
    ref.set_weights(w0)
    return ref, w0
