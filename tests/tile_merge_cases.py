"""The nets, data sets and call schedules on which the merged tile map's workgroup kinds (csrc/tile_step_body.inc: a group of layer
0's partial last tile row, a pair of a later layer) are compared with their GNN_MLP_TILE_MERGE=0 twin and the fp64 oracle
(tests/test_tile_merge_cases_cpu.py pins the properties; tests/test_tile_merge_cases_gpu.py runs them on the device).

A case is a shape, a net class (softmax / cross entropy, or last activation + half squared loss), an inner activation, max_batch
and a schedule: a list of calls on one handle, at most 15 gradient steps (a lone handle instantiates its row kernels at its 16th
gradient computation; that crossing belongs to tests/test_chain_shapes_gpu.py).  A call is one of
    ("range", first, B, n)          train_range(first, B, n)
    ("sampled", n, B)               gnn_mlp_train_sampled: n draws of B from the handle's sampler (seed SAMPLER_SEED)
    ("step", first, B, hint)        hint_next_range(*hint) unless hint is None, then gradient_step_range(first, B)
and `recut` holds the same gradient steps cut into calls differently (None: the case has no second cut).

max_batch is 304 on every small case: the largest padded batch the schedules use, and every shape here keeps step_launches == 2
with it (asserted on the device).  The 784- and 800-wide shapes run 6 + 6 steps of train_range on handles of max_batch 128.

Shapes.  The planted ones are listed with what they plant in PLANTED; two notes on them:
  * 784-304-96-16 is a second map with 32 entries on the fullest XCD and an even column count in layer 1 (pairs only).  The
    wider 784-304-128-16 would give the same map but does not pass make_rb_plan (its LDS images need 202 KB), so it would never
    launch the merged kinds;
  * 20 inputs pad to 32, so 20-300-100-10 has 32-row groups (nine of 2 columns and one of 1), not 16-row groups of 4, 4, 4, 4, 3;
    it stays, and 12-300-100-10 carries the 16-row reading (no whole tile, groups 4, 4, 4, 4, 3).
The eight drawn shapes come from d0 in [1, 400), 3..6 layers, middle widths <= 384, last hidden width <= 128, outputs in [2, 17),
redrawn until rb_ok() -- a restatement of make_rb_plan's conditions that the CPU test holds against the real one."""
from collections import namedtuple

import numpy as np

from tests import chain_cases as cc
from tests import np_oracle

OUT_SOFTMAX_CE, OUT_ACT_LOSS = cc.OUT_SOFTMAX_CE, cc.OUT_ACT_LOSS
STEP, MOMENTUM, SAMPLER_SEED, W_SCALE = cc.STEP, cc.MOMENTUM, cc.SAMPLER_SEED, cc.W_SCALE
W_ATOL = 2e-6            # per step, weights and momentum, f32 against fp64: the bound of test_chain_shapes_gpu.py and test_trainer_gpu.py
MAX_BATCH = 304
MAX_STEPS = 15
TM, TN, PAD = 64, 16, 16  # the tile kernel's tile (TS_TM x TS_TN) and the padding of every width and batch
N_ROWS = 600             # data set of the range and announced schedules: a multiple of 1, 100, 120 and 300 (a batch ends at its last row)

PLANTED = [
    ([1, 17, 10], "layer 0 is one 16-row group of 2 columns; one live weight row; no whole tile"),
    ([16, 16, 2], "a group of 1 column; the whole net is two workgroups"),
    ([20, 300, 100, 10], "no whole tile; 32-row groups 9 x 2 + 1; layer 1: 304 rows = 4 x 64 + 48, 7 columns (pairs 2, 2, 2 + single)"),
    ([12, 300, 100, 10], "no whole tile; 16-row groups 4, 4, 4, 4, 3"),
    ([32, 33, 10], "32-row only row, 3 columns: groups 2 + 1"),
    ([33, 48, 10], "48-row only row: counts as whole, regular slots"),
    ([65, 100, 70, 10], "one live row of a 16-row group; layer 1 a 48-row partial row of pairs + a single, layer 2 a 16-row partial row of a single"),
    ([90, 112, 80, 5], "26 live rows of a 32-row group; layer 1 a 48-row partial row of pairs + a single"),
    ([80, 96, 16], "16-row groups 4 + 2; layer 1 has a 32-row partial tile row"),
    ([80, 80, 10], "16-row groups 4 + 1"),
    ([96, 64, 10], "32-row groups, full only (2 + 2)"),
    ([129, 16, 16, 16, 16, 2], "six layers, every layer one column wide"),
]
# every schedule kind runs on these (a 16-row group, a 32-row group, and pairs on a partial tile row of a later layer among them)
CARRIERS = [[65, 100, 70, 10], [90, 112, 80, 5], [20, 300, 100, 10]]
HEADLINE = [[784, 300, 100, 10], [784, 304, 96, 16], [784, 100, 50, 10]]
NOT_USABLE = [800, 300, 100, 10]     # 33 entries on one XCD of 32 CUs: the one-tile map, tile_merge_state == 0
N_DRAWN = 8
KINDS = ["sizes", "announced", "sampled_small", "sampled_large"]

Case = namedtuple("Case", "name dims out_kind inner last max_batch rows kind schedule recut seed wseed")


def pad(n):
    return (n + PAD - 1) // PAD * PAD


def rb_ok(dims):
    """make_rb_plan(dims).ok (csrc/rowblock_kernel.h), restated: the conditions under which the two-launch step trains with the
    row-block kernel -- and only then launches the merged kinds."""
    L = len(dims)
    if L < 3 or L > 8:
        return False
    ld = [pad(d) for d in dims]
    kr = [(d + 3) // 4 * 4 for d in dims]
    Lm = L - 1
    if ld[Lm] != 16 or kr[Lm - 1] > 128 or any(ld[l] > 1024 for l in range(1, Lm)) or (ld[0] + 63) // 64 > 16 or ld[1] > 512:
        return False
    off = 0
    for l in range(1, Lm):
        lw4 = kr[l + 1] // 4
        off += kr[l] * 4 * (lw4 + 1 - lw4 % 2)
    off += sum(4 * (ld[l] + 4) for l in range(1, Lm)) + sum(4 * (ld[l] + 4) for l in range(2, Lm + 1)) + 4 * ld[Lm] + 4 * (ld[1] + 4)
    scratch = 0
    for l in range(1, Lm - 1):
        cs = 1
        while cs * 128 < ld[l + 1]:
            cs *= 2
        if cs > 8:
            return False
        ksf = 8 // cs
        if (ld[l] // 8 + ksf - 1) // ksf > 6:
            return False
        scratch = max(scratch, ksf * 4 * ld[l + 1])
    return (off + scratch + 64) * 4 <= 160 * 1024 - 256


def drawn_dims(i):
    """Drawn shape i (0..7): redrawn from the same generator until rb_ok."""
    rng = np.random.default_rng(9100 + i)
    while True:
        L = int(rng.integers(3, 7))
        dims = [int(rng.integers(1, 400))] + [int(rng.integers(1, 129 if j == L - 3 else 385)) for j in range(L - 2)] + [int(rng.integers(2, 17))]
        if rb_ok(dims):
            return dims


def partial_row_inputs(dims):
    """The input columns whose weights lie in layer 0's partial last tile row (16 or 32 padded rows: the groups); without such a row,
    the inputs of layer 0's last tile row."""
    m0 = (pad(dims[0]) - 1) // TM * TM
    return np.arange(m0, dims[0])


# ---- schedules ---------------------------------------------------------------------------------------------------------------
def sizes_schedule():
    """train_range at every batch size class on one handle, 15 steps: 1, 16, 100 (ragged below 112), 120 (K = 128 with dead rows),
    128, 136 (129..143), 144, 256 (two whole K chunks), 300 (two chunks and a ragged one).  The walks of 1, 100 and 120 rows start at
    the batch that ends at the data set's last row and wrap; 300 ends there too.  recut: every step a call of its own."""
    calls = [("range", 599, 1, 2), ("range", 576, 16, 2), ("range", 500, 100, 2), ("range", 480, 120, 2), ("range", 384, 128, 2),
             ("range", 0, 136, 1), ("range", 432, 144, 1), ("range", 256, 256, 2), ("range", 300, 300, 1)]
    recut = [("range", r, B, 1) for _, first, B, n in calls for r in cc.range_batches(N_ROWS, B, first, n)]
    return N_ROWS, calls, recut


def announced_schedule():
    """hint_next_range + gradient_step_range, 14 steps: consecutive batches whose padded sizes differ in both directions across
    128 (16 -> 144 -> 16 -> 120 -> 128 -> 300 -> 100 -> 256 -> 1 -> 136 -> 130 -> 128 -> 16 -> 144), starting anywhere, the one of
    120 rows ending at the data set's last row.  The announcement in front of a step names the batch of the step AFTER it; the
    ones in front of steps 3 and 9 name another batch (and must go unused: the step after starts from a forward-only launch), the
    last step announces nothing.  recut: the same steps unannounced."""
    sizes = [16, 144, 16, 120, 128, 300, 100, 256, 1, 136, 130, 128, 16, 144]
    walk = [((N_ROWS - n) if n == 120 else (s * 97) % (N_ROWS - n + 1), n) for s, n in enumerate(sizes)]
    calls = []
    for s, (first, n) in enumerate(walk):
        hint = walk[s + 1] if s + 1 < len(walk) else None
        if s in (3, 9):
            hint = (hint[0] // 2 + 1, n)     # another first row AND another size than the batch that follows
        calls.append(("step", first, n, hint))
    return N_ROWS, calls, [("step", first, n, None) for first, n in walk]


def sampled_schedule(B):
    """train_sampled, 9 draws of B from 3 B + B // 2 + 1 rows in calls of 5 + 4: the sampler refills inside the fourth draw, which
    comes out shorter than B (NNT:143-168).  recut: 2 + 7."""
    return 3 * B + B // 2 + 1, [("sampled", 5, B), ("sampled", 4, B)], [("sampled", 2, B), ("sampled", 7, B)]


def headline_schedule():
    """6 steps of train_range at 128 and 6 at 120 (K = 128 with 8 dead rows; the second batch ends at the data set's last row)."""
    return N_ROWS, [("range", 0, 128, 6), ("range", 360, 120, 6)], None


def _schedule(kind):
    return {"sizes": sizes_schedule, "announced": announced_schedule, "sampled_small": lambda: sampled_schedule(100),
            "sampled_large": lambda: sampled_schedule(144), "headline": headline_schedule}[kind]()


# ReLU (3) has a zero derivative: a hidden unit that no row of a batch drives above zero gets no gradient in that step, so a ReLU
# net meets "every weight moves, every unit of layer 1 feeds a gradient into the groups in every step" only by luck of its weights
# and data.  The draw gives ReLU to seven sampled_large cases; on these two a re-seed (data seed + 100 j, weight seed 1 + j, the
# first j of 1..11 that meets it in the fp64 oracle: j = 11 and j = 2) does, the other five run leaky ReLU instead.
RESEEDED = {"96-64-10-sampled_large": (4019 + 1100, 12), "68-116-15-sampled_large": (4023 + 200, 3)}   # name -> (data seed, weight seed)


def _net_of(i, name):
    """Net class and activations of case i: the four inner activations in turn (ReLU only on the cases of RESEEDED), every third
    case a GeneralNeuralNet with each last activation in turn."""
    inner = i % 4
    if inner == 3 and name not in RESEEDED:
        inner = 0
    out_kind = OUT_ACT_LOSS if i % 3 == 1 else OUT_SOFTMAX_CE
    return out_kind, inner, cc.LAST_ACTS[(i // 3) % 3]


def _cases():
    specs = [(d, k) for d in CARRIERS for k in KINDS]
    others = [d for d, _ in PLANTED if d not in CARRIERS] + [drawn_dims(i) for i in range(N_DRAWN)]
    specs += [(d, KINDS[j % 4]) for j, d in enumerate(others)]
    specs += [(d, "headline") for d in HEADLINE + [NOT_USABLE]]
    out = []
    for i, (dims, kind) in enumerate(specs):
        rows, calls, recut = _schedule(kind)
        name = "%s-%s" % ("-".join(map(str, dims)), kind)
        out_kind, inner, last = _net_of(i, name)
        out.append(Case(name, list(dims), out_kind, inner, last, 128 if kind == "headline" else MAX_BATCH,
                        rows, kind, calls, recut, *RESEEDED.get(name, (4000 + i, 1))))
    return out


CASES = _cases()
IDS = [c.name for c in CASES]


# ---- data, the oracle's trajectory ---------------------------------------------------------------------------------------------
def case_data(case):
    """X and one-hot Y.  Half of X's entries are zero, except in the inputs of layer 0's partial tile row: those are at least
    0.05 in every row, so that every batch -- of one row too -- puts a non-zero operand into every weight row of the groups."""
    rng = np.random.default_rng(case.seed)
    d0 = case.dims[0]
    X = rng.random((case.rows, d0)) * (rng.random((case.rows, d0)) < 0.5)
    cols = partial_row_inputs(case.dims)
    X[:, cols] = 0.05 + 0.95 * rng.random((case.rows, cols.size))
    Y = np.eye(case.dims[-1])[rng.integers(0, case.dims[-1], case.rows)]
    return X, Y


def oracle_net(oracle_mod, case):
    """The case's net in the fp64 C oracle with the case's start weights (the Random(1) draw as f32, times W_SCALE: exact in f32)."""
    ref = oracle_mod.OracleNet(case.dims, out_kind=case.out_kind, inner_act=case.inner, last_act=case.last, seed=case.wseed)
    ref.set_alloc_per_sample(0)
    w0 = ref.get_weights().astype(np.float32).astype(np.float64) * W_SCALE
    ref.set_weights(w0)
    return ref, w0


def call_batches(oracle_mod, case, calls):
    """Per call, the row indices of each of its gradient steps (sampled calls: the oracle sampler's draws, one sampler per handle)."""
    smp = oracle_mod.Sampler(case.rows, seed=SAMPLER_SEED)
    out = []
    for call in calls:
        if call[0] == "range":
            _, first, B, n = call
            out.append([np.arange(r, r + B) for r in cc.range_batches(case.rows, B, first, n)])
        elif call[0] == "sampled":
            out.append([smp.sample(call[2]) for _ in range(call[1])])
        else:
            out.append([np.arange(call[1], call[1] + call[2])])
    return out


def n_steps(calls):
    return sum(c[3] if c[0] == "range" else c[1] if c[0] == "sampled" else 1 for c in calls)


def trajectory(oracle_mod, case, observe=None):
    """The schedule in the fp64 oracle; returns (w0, weights, momentum) at its end.  observe(ref, X[idx], Y[idx]) runs before every step."""
    X, Y = case_data(case)
    ref, w0 = oracle_net(oracle_mod, case)
    for batches in call_batches(oracle_mod, case, case.schedule):
        for idx in batches:
            if observe:
                observe(ref, X[idx], Y[idx])
            ref.gradient_step(X[idx], Y[idx], STEP, MOMENTUM)
    w, v = ref.get_weights(), ref.get_momentum()
    ref.close()
    return w0, w, v


def trajectory_f32(oracle_mod, case):
    """The schedule restated in float32 numpy (tests/np_oracle.py): what the reference alone is away from itself in f32."""
    X, Y = case_data(case)
    _, w0 = oracle_net(oracle_mod, case)
    w, v = w0.astype(np.float32), np.zeros(w0.size, dtype=np.float32)
    for batches in call_batches(oracle_mod, case, case.schedule):
        for idx in batches:
            w, v = np_oracle.gradient_step(w, v, case.dims, X[idx], Y[idx], STEP, MOMENTUM, case.inner, case.out_kind, case.last, dtype=np.float32)
    return w, v


# ---- the host checker (tests/native/tile_merge_check.hip) ------------------------------------------------------------------------
def build_checker(directory):
    """Compiles the checker into `directory`; None without hipcc."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return None
    out = os.path.join(str(directory), "tile_merge_check")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-o", out, os.path.join(root, "tests", "native", "tile_merge_check.hip")],
                   check=True, capture_output=True, timeout=600)
    return out


Entry = namedtuple("Entry", "id layer row col kind height cols live_rows")
WHOLE, GROUP, PAIR, SINGLE = 0, 1, 2, 3


def entries(checker, dims, cus_per_xcd):
    """(entries, summary) of the checker's per-entry report: summary holds rb_ok, usable, grid, max_xcd, ..."""
    import subprocess
    r = subprocess.run([checker, "entries", str(cus_per_xcd)] + [str(d) for d in dims], check=True, capture_output=True, text=True, timeout=60)
    lines = r.stdout.strip().split("\n")
    f = lines[-1].split()
    return [Entry(*map(int, ln.split()[1:])) for ln in lines[:-1]], dict(zip(f[0::2], map(int, f[1::2])))
