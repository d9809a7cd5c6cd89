"""The seeded draw of CALL SEQUENCES and their fp64 model (tests/test_sequence_cases_cpu.py pins the properties of the draw and
the power of the budgets; tests/test_call_sequences_gpu.py runs the sequences on the device).  No GPU and no product code: numpy,
tests/np_oracle.py and the C oracle only.

What is under test is the HOST bookkeeping that decides which device buffers a kernel may trust (csrc/lookahead.h, PendingUpdate
in csrc/plan.hip, EvalScope, enter_grouped / leave_grouped in csrc/group.hip, the shared gradient buffer, the bf16 shadow of the
weights): a state that stays valid once too often feeds a kernel sums of replaced weights, rows of a replaced data set or padding
rows of a larger batch, and the result is silently wrong.  One handle (or one group) receives a drawn sequence of calls from the
whole ABI vocabulary; a random order alone would rarely hit the dangerous pairs, so the draw PLANTS them (H1 .. H10, `hazards()`),
shuffles the planted blocks and fills the gaps from the rest of the vocabulary.

A sequence is a list of ops `(name, kwargs)`:
  training  step_host  step_range  step_indexed  train_range  train_sampled  train_observed  compute_gradient_range  apply_update  hint
  reading   propagate  loss  argmax  loss_range  argmax_range  count_hits  evaluate  confusion  labels  weight_gradient
            get_weights  get_momentum  save
  writing   set_weights  set_momentum  load  upload  specialize  forget  advance_time  timing  synchronize  sample
  refused   refused(kind = batch | step | rows | validation)
and, for groups (group_case), g_train_range, g_train_sampled (mode = shared | each | sizes), g_train_observed, g_evaluate, g_confusion,
g_ensemble, g_upload and `member` (k, one of the lone ops above, or refused(kind = upload)).

Sizes: max_batch = 40 for every net; batch sizes from BATCHES, so a handle sized for 40 rows keeps seeing batches that fall short of
its buffers by less and by more than a 16-row pad; data sets of 101 rows, re-uploads of 101 (other rows), 57 or 130 rows; steps of
chain_cases.STEP / MOMENTUM (the project's per-step budget is stated for steps of that size); start weights = the Random(1) draw
times chain_cases.W_SCALE; set_weights puts the f32-rounded NEGATED Random(2) draw times the same scale -- far from anything the
handle held.

`Model` applies an op list as the reference defines each call (OracleNet for steps, losses and argmax, plain numpy for apply_update,
SCE:324-344, on the gradient it recorded) and, given one of FAULTS, as a handle with that bookkeeping mistake would:
  F1 stale first-layer sums after a weight replacement          F5 rows of the previous, larger batch (up to the 16-row pad) counted
  F2 the pending update dropped when a non-step call follows       in a short batch's gradient
  F3 the pending update applied AFTER set_weights / set_momentum / F6 momentum not restored by load_checkpoint
     load_checkpoint instead of before                           F7 a step on the old data set's rows after an upload
  F4 the exported gradient added to the next step's              F8 the bf16 forward on the shadow of the replaced weights
Least distance of a faulty model from the correct one at the FIRST check behind the hazard (a checkpoint, or a get_weights /
get_momentum in front of it), in budgets, over the lone sequences (tests/test_sequence_cases_cpu.py asserts >= 2 for every sequence
and prints them): F1 7.22, F2 83.9, F3 42, F4 36.5, F5 37.9, F6 85.7, F7 12.5, F8 29.4 (FAULT_FACTORS_FOUND).  What moved the
draw there: load_checkpoint behind a hinted step restores slot 0 after a set_weights (a checkpoint two steps old leaves stale sums
nearly right: 1.68); weights and momentum are also compared in front of every load_checkpoint (it wipes a fault's trace); the
exported gradient is of 33 or 40 rows and the step behind it of 3 to 5 (1.79 otherwise) with a get_weights behind it; the host-batch
step in front of a load_checkpoint has 40 rows; the bf16 shadow is looked at by a propagate right behind a replacement.

Length: a lone sequence has about 100 calls and 75 to 83 steps (every planted block costs three to five calls; one sampled loop of
17 to 20 iterations crosses the sampler's first chunk of 16), a group sequence 34; on the MI355X every case, lone or group, takes less than 2.3 s."""
import functools

import numpy as np

from tests import chain_cases as cc
from tests import np_oracle

MAX_BATCH = 40
BATCHES = (1, 3, 4, 5, 15, 16, 17, 33, 40)
ROWS, REUPLOAD_ROWS = 101, (57, 130)
HOST_ROWS = 64                 # the pool host batches are cut from
SEEDS_PER_NET = 3
CHECK_EVERY = 8                # weights and momentum are compared every 8 ops and at the end
SAMPLER_SEED = cc.SAMPLER_SEED
W_ATOL = 2e-6                  # per step so far, weights and momentum, f32 against fp64 (tests/test_trainer_gpu.py)
OUT_ATOL = 2e-4                # outputs (tests/test_parity_gpu.py, P_ATOL)
LOSS_RTOL = LOSS_ATOL = 2e-4   # losses and validation values (tests/test_parity_gpu.py)
# Two f32 evaluations of ONE loss by kernels that add the same products in another order (a grouped launch against the lone net's):
# a layer's dot product of d <= 1025 terms accumulates about sqrt(d) <= 32 roundings of 2^-24 each, i.e. 16 ulp of 2^-23 on its
# logits, which enter the loss absolutely (|dl| <= |dz|, logits of size O(1)) and relatively -- per row 16 * 2^-23 * (1 + |l|).
# tests/test_sequence_cases_cpu.py shows that a validation pass on weights one step old leaves it by a factor of 2 or more.
ORDER_ULPS = 16 * 2.0 ** -23


def order_bound(loss_sum, n):
    """the bound above for a sum of n rows' losses"""
    return ORDER_ULPS * (n + abs(loss_sum))
MARGIN = {cc.OUT_SOFTMAX_CE: 1e-3, cc.OUT_ACT_LOSS: 1e-4}   # top-2 margin of a row whose label must be exact: logits / General outputs
SAFE_SHARE = 0.9               # of the rows at every label check (tests/test_general_net_gpu.py)
BF16_OUT, BF16_W = 5e-3, {3: 2e-4, 5: 4e-4}                 # bf16: outputs; weights and momentum after 3 / 5 steps (test_chained_loops_bf16)
FAULTS = ("F1", "F2", "F3", "F4", "F5", "F6", "F7", "F8")
FAULT_FACTORS_FOUND = {"F1": 7.22, "F2": 83.9, "F3": 42.0, "F4": 36.5, "F5": 37.9, "F6": 85.7, "F7": 12.5, "F8": 29.4}

TRAINING = ("step_host", "step_range", "step_indexed", "train_range", "train_sampled", "train_observed")
REPLACING = ("set_weights", "load")
EVALS = ("count_hits", "evaluate", "confusion", "labels")
H3_FOLLOWERS = ("get_weights", "propagate", "eval_above", "save", "set_weights", "set_momentum", "load", "refused", "step_range",
                "train_sampled", "compute_gradient_range")
LEAKY, SIGMOID, TANH, RELU, IDENT = range(5)


def _chain(seed):
    dims, _, inner, out_kind, last = cc.chain_case(seed)
    return dims, inner, out_kind, last


# The eight lone nets, chosen by the path they take (tests/test_call_sequences_gpu.py asserts each class from step_launches,
# rowblock_state, specialization and plan_note): name, dims, inner, out_kind, last, dtype
NETS = [
    ("f32-rowblock",) + _chain(4) + ("f32",),                    # 784-91-16: two launches, row-block kernel, runtime shape
    ("f32-middle4",) + _chain(19) + ("f32",),                    # 243-20-76-29: 29 outputs, middle4_kernel as the row kernel
    ("f32-three-launch",) + _chain(7) + ("f32",),                # input width 1025: 17 first-layer K slabs
    ("f32-per-layer", [300, 10], LEAKY, cc.OUT_SOFTMAX_CE, IDENT, "f32"),
    ("f32-prebuilt", [784, 100, 50, 10], LEAKY, cc.OUT_SOFTMAX_CE, IDENT, "f32"),
    ("f32-general",) + _chain(14) + ("f32",),                    # 556-105-12, GeneralNeuralNet, sigmoid / identity
    ("bf16-rowblock",) + _chain(18) + ("bf16",),                 # 890-166-78-15
    ("bf16-middle4",) + _chain(12) + ("bf16",),                  # 573-14-97-12-67-7
]
N_LONE = len(NETS) * SEEDS_PER_NET
# the seed of a sequence's DATA where the sequence's own left fewer than 90 % of the rows safe at one of its label checks
DATA_SEEDS = {23: 8123}


def lone_case(i):
    """Sequence i of the 24: net i // 3, draw seed i % 3."""
    name, dims, inner, out_kind, last, dtype = NETS[i // SEEDS_PER_NET]
    seed = 9100 + i
    return dict(id="%s-%d" % (name, i % SEEDS_PER_NET), net=name, dims=list(dims), inner=inner, out_kind=out_kind, last=last, dtype=dtype,
                seed=DATA_SEEDS.get(i, seed), draw_seed=seed, ops=draw_ops(seed))


# ---- data -----------------------------------------------------------------------------------------------------------------------
def _rows(seed, n, d_in, d_out):
    rng = np.random.default_rng(seed)
    X = (rng.random((n, d_in)) * (rng.random((n, d_in)) < 0.5)).astype(np.float32).astype(np.float64)   # (as the device holds them)
    Y = np.eye(d_out)[rng.integers(0, d_out, n)]
    X.setflags(write=False); Y.setflags(write=False)
    return X, Y


def rows_of(which):
    """0, 1: 101 rows; 57, 130: a re-upload of that size; 1057, 1130: other rows of that size"""
    return ROWS if which in (0, 1) else which % 1000


@functools.lru_cache(maxsize=64)
def dataset(seed, which, d_in, d_out):
    """Data set `which` of a sequence (rows_of)"""
    return _rows(31 * seed + which, rows_of(which), d_in, d_out)


@functools.lru_cache(maxsize=64)
def host_pool(seed, d_in, d_out):
    return _rows(31 * seed + 7, HOST_ROWS, d_in, d_out)


def start_weights(oracle_mod, dims, seed=1):
    """The Random(seed) draw times W_SCALE, f32-exact (the product holds f32 masters)"""
    return oracle_mod.OracleNet(dims, seed=seed).get_weights().astype(np.float32).astype(np.float64) * cc.W_SCALE


def replacement_weights(oracle_mod, dims):
    return (-start_weights(oracle_mod, dims, seed=2)).astype(np.float32).astype(np.float64)


def replacement_momentum(oracle_mod, dims):
    """set_momentum's vector: the Random(3) draw at the size of a step's update"""
    return (start_weights(oracle_mod, dims, seed=3) * 0.01).astype(np.float32).astype(np.float64)


# ---- the draw -------------------------------------------------------------------------------------------------------------------
class _Draw:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.ops = []
        self.N = ROWS
        self.saves = 0
        self.evals = [EVALS[int(i)] for i in self.rng.permutation(len(EVALS))]

    def eval_kind(self):
        """the four evaluation calls in turn"""
        self.evals.append(self.evals.pop(0))
        return self.evals[-1]

    def add(self, name, **kw):
        self.ops.append((name, kw))

    def pick(self, xs):
        return xs[int(self.rng.integers(0, len(xs)))]

    def first(self, B):
        return int(self.rng.integers(0, self.N - B + 1))

    def host(self, n):
        return dict(off=int(self.rng.integers(0, HOST_ROWS - n + 1)), n=n)

    def idx(self, n):
        return dict(idx=[int(i) for i in self.rng.permutation(self.N)[:n]])

    def slot(self):
        return int(self.rng.integers(0, self.saves))

    def above(self):
        """an evaluation of more rows than max_batch: the workspace swap"""
        n = int(self.rng.integers(MAX_BATCH + 1, self.N + 1))
        return self.eval_kind(), dict(first=int(self.rng.integers(0, self.N - n + 1)), n=n)

    def below(self):
        n = self.pick(BATCHES)
        return self.eval_kind(), dict(first=self.first(n), n=n)

    def range_call(self, n_steps=None):
        """train_range arguments and the batch its last step prepares"""
        B = self.pick([b for b in (15, 16, 17, 33, 40) if self.N // b >= 2])
        nb = self.N // B
        b0 = int(self.rng.integers(0, nb))
        n = int(self.rng.integers(1, 6)) if n_steps is None else n_steps
        return dict(first=b0 * B, B=B, n_steps=n), (((b0 + n) % nb) * B, B)

    def filler(self, r):
        n = self.pick(BATCHES)
        if r == 0: self.add("loss", **self.host(n))
        elif r == 1: self.add("argmax", **self.host(n))
        elif r == 2: self.add("loss_range", first=self.first(n), n=n)
        elif r == 3: self.add("argmax_range", first=self.first(n), n=n)
        elif r == 4: _add(self, self.above())
        elif r == 5: _add(self, self.below())
        elif r == 6:
            k = int(self.rng.integers(1, 9))
            self.add("advance_time", n=k); self.add("advance_time", n=-k)
        elif r == 7: self.add("synchronize")
        else: self.add("forget")


N_FILLERS = 9


def _add(d, pair):
    d.ops.append((pair[0], pair[1]))


def _h3(d, follower, n=None):
    """a host-batch step immediately followed by `follower` (its update is pending when the follower arrives)"""
    n = (MAX_BATCH if follower == "load" else d.pick(BATCHES)) if n is None else n     # (load wipes a short batch's trace: a full one)
    d.add("step_host", **d.host(n))
    if follower == "get_weights": d.add("get_weights")
    elif follower == "propagate": d.add("propagate", **d.host(d.pick(BATCHES)))
    elif follower == "eval_above": _add(d, d.above())
    elif follower == "save": d.add("save", slot=d.saves); d.saves += 1
    elif follower == "set_weights": d.add("set_weights"); d.add("propagate", **d.host(5))
    elif follower == "set_momentum": d.add("set_momentum")
    elif follower == "load": d.add("load", slot=d.slot()); d.add("propagate", **d.host(17))
    elif follower == "refused": d.add("refused", kind=d.pick(["batch", "step", "rows", "validation"]))
    elif follower == "step_range":
        m = d.pick(BATCHES); d.add("step_range", first=d.first(m), n=m)
    elif follower == "train_sampled": d.add("train_sampled", iters=int(d.rng.integers(1, 4)), B=d.pick([5, 16, 33]))
    elif follower == "compute_gradient_range":
        m = d.pick(BATCHES); f = d.first(m)
        d.add("compute_gradient_range", first=f, n=m)
        if d.rng.random() < 0.5: d.add("loss_range", first=d.first(4), n=4)      # another op between the gradient and its update
        d.add("apply_update", B=m)


def _blocks():
    """The planted blocks, each a function of the draw state; H3's followers and the refusals ride in several of them."""
    def h1_loop(d):       # H1: a loop leaves sums for batch b; set_weights; a step on exactly b
        call, nxt = d.range_call()
        d.add("train_range", **call); d.add("set_weights"); d.add("step_range", first=nxt[0], n=nxt[1])

    def h1_hint(d):       # H1: a rightly hinted step leaves sums for the hinted batch; load_checkpoint; a step on it
        b1, b2 = d.pick(BATCHES), d.pick((15, 16, 17, 33))
        f2 = d.first(b2)
        d.add("set_weights")                                  # (far from slot 0, the start weights five steps on)
        d.add("hint", first=f2, n=b2); d.add("step_range", first=d.first(b1), n=b1)
        d.add("load", slot=0); d.add("step_range", first=f2, n=b2)

    def h2_same(d):       # H2: sums for (first, B); the data set replaced by other rows of the same count; a step on (first, B)
        call, nxt = d.range_call()
        d.add("train_range", **call); d.add("upload", which=1 if d.N == ROWS else 1000 + d.N); d.add("step_range", first=nxt[0], n=nxt[1])

    def h2_resize(d):     # H2 with another row count (the sampler of the old size goes with the old rows)
        which = d.pick(REUPLOAD_ROWS)
        B = d.pick((15, 16, 17))
        d.add("hint", first=B, n=B); d.add("step_range", first=0, n=B)
        d.add("upload", which=which); d.N = which
        d.add("step_range", first=B, n=B)

    def h4(d):            # H4: an exported gradient (of many rows), then an ordinary step (on few: the fault's share is large)
        n, m = d.pick((33, 40)), d.pick((3, 4, 5))
        d.add("weight_gradient", **d.host(n)); d.add("step_range", first=d.first(m), n=m); d.add("get_weights")
        d.add("compute_gradient_range", first=d.first(n), n=n); d.add("step_host", **d.host(m)); d.add("get_momentum")

    def h5(d):            # H5: an evaluation of n > max_batch rows between two steps of one chain
        call, nxt = d.range_call(2)
        d.add("train_range", **call); _add(d, d.above())
        d.add("train_range", first=nxt[0], B=nxt[1], n_steps=int(d.rng.integers(1, 4)))

    def h6_range(d):      # H6: 33 or 40 rows, then 3 or fewer, then 17
        a, b = d.pick((33, 40)), d.pick((1, 3))
        d.add("step_range", first=d.first(a), n=a); d.add("step_range", first=d.first(b), n=b); d.add("step_range", first=d.first(17), n=17)

    def h6_index(d):
        a, b = d.pick((33, 40)), d.pick((1, 3))
        d.add("step_indexed", **d.idx(a)); d.add("step_indexed", **d.idx(b)); d.add("step_indexed", **d.idx(17))

    def h6_host(d):       # ... by host batch, each step with one of H3's followers behind it
        _h3(d, "eval_above", d.pick((33, 40))); _h3(d, "set_momentum", d.pick((1, 3))); _h3(d, "get_weights", 17)

    def h7(d):            # H7: a sampled loop, a host sample(), an observed loop on the same sampler; refills inside batches
        # (csrc/sample_ring.h: chunks of 16, 32, .. iterations -- 17 to 20 iterations cross the first chunk's end, so the next
        #  chunk's upload and the chain through the boundary are in play, and end inside the second)
        d.add("train_sampled", iters=int(d.rng.integers(17, 21)), B=d.pick((15, 17)))
        d.add("sample", B=d.pick(BATCHES))
        d.add("train_observed", iters=int(d.rng.integers(2, 5)), B=d.pick((17, 33)), V=d.pick((7, 16)))
        d.add("sample", B=3)
        d.add("train_observed", iters=2, B=d.pick((4, 16)), V=int(d.rng.integers(MAX_BATCH + 1, d.N + 1)))

    def h8(d):            # H8: specialize() between two chained steps
        b1, b2 = d.pick(BATCHES), d.pick(BATCHES)
        f2 = d.first(b2)
        d.add("hint", first=f2, n=b2); d.add("step_range", first=d.first(b1), n=b1); d.add("specialize"); d.add("step_range", first=f2, n=b2)

    def h9(d):            # H9: apply_update followed by a chained step
        b1, b2 = d.pick(BATCHES), d.pick(BATCHES)
        f2 = d.first(b2)
        d.add("compute_gradient_range", first=d.first(b1), n=b1); d.add("hint", first=f2, n=b2)
        d.add("apply_update", B=b1 * int(d.rng.integers(1, 3))); d.add("step_range", first=f2, n=b2)

    def h10(d):           # H10: timing toggled inside a chain
        B = d.pick((16, 17, 33))
        f = [d.first(B) for _ in range(3)]
        d.add("hint", first=f[1], n=B); d.add("step_range", first=f[0], n=B); d.add("timing", on=True)
        d.add("hint", first=f[2], n=B); d.add("step_range", first=f[1], n=B); d.add("timing", on=False)
        d.add("step_range", first=f[2], n=B)

    def wrong_hint(d):    # a hint that names another batch than the one that follows, and one never used
        B = d.pick(BATCHES)
        d.add("hint", first=d.first(B), n=B); d.add("step_range", first=d.first(17), n=17)
        d.add("hint", first=d.first(B), n=B); _h3(d, "step_range")

    def refusals(d):
        for kind in ("batch", "step", "rows", "validation"):
            d.add("refused", kind=kind)
        d.add("step_range", first=d.first(5), n=5)

    followers = [lambda d, f=f: _h3(d, f) for f in H3_FOLLOWERS if f not in ("eval_above", "set_momentum", "get_weights")]
    return [h1_loop, h1_hint, h2_same, h2_resize, h4, h5, h6_range, h6_index, h6_host, h7, h8, h9, h10, wrong_hint, refusals] + followers


def draw_ops(seed, with_starts=False):
    """The lone sequence of `seed`: a prologue that reaches 3 and 5 steps at op boundaries (the bf16 budgets exist for those) and
    saves a checkpoint, then every planted block in a drawn order with drawn fillers between them."""
    d = _Draw(seed)
    d.add("train_range", first=0, B=17, n_steps=3); d.add("get_weights")
    d.add("step_host", **d.host(16)); d.add("save", slot=0); d.saves = 1
    d.add("step_range", first=d.first(33), n=33); d.add("get_momentum")
    blocks = _blocks()
    fillers = [int(r) for r in d.rng.permutation(N_FILLERS)]
    d.starts = []                                              # where each planted block begins
    for i in d.rng.permutation(len(blocks)):
        d.starts.append(len(d.ops))
        blocks[int(i)](d)
        if fillers and d.rng.random() < 0.6:
            d.filler(fillers.pop())
    while fillers:
        d.filler(fillers.pop())
    return (d.ops, d.starts) if with_starts else d.ops


# ---- the hazards a sequence contains ----------------------------------------------------------------------------------------------
def _rows_of(op):
    name, kw = op
    if name in ("step_host", "step_range", "compute_gradient_range"): return kw["n"]
    if name == "step_indexed": return len(kw["idx"])
    return None


def _is_above(op):
    return op[0] in EVALS and op[1]["n"] > MAX_BATCH


def hazards(ops):
    """{hazard: [op indices]} of a lone sequence, from the op list alone: H1 and H2 by following which batch has sums made ahead
    (a train_range's last step prepares the batch behind the range; a step prepares the hinted batch), the others by pattern."""
    found = {}
    def hit(h, i): found.setdefault(h, []).append(i)
    ahead, hint, replaced, uploaded, N, exported = None, None, False, False, ROWS, False
    for i, (name, kw) in enumerate(ops):
        prev = ops[i - 1] if i else ("", {})
        nxt = ops[i + 1] if i + 1 < len(ops) else ("", {})
        key = None
        if name == "step_range": key = (kw["first"], kw["n"])
        if name == "train_range": key = (kw["first"], kw["B"])
        if key is not None and ahead == key:
            if replaced: hit("H1", i)
            if uploaded: hit("H2", i)
        if name in TRAINING and exported: hit("H4", i)
        if name in TRAINING or name in ("weight_gradient", "apply_update"): exported = False
        if name == "weight_gradient" or (name == "compute_gradient_range" and nxt[0] != "apply_update" and ops[min(i + 2, len(ops) - 1)][0] != "apply_update"):
            exported = True
        # one chain: a step that starts on the batch the step before it prepared
        if key is not None and ahead == key and not replaced and not uploaded:
            if _is_above(prev): hit("H5", i)
            if prev[0] == "specialize": hit("H8", i)
            if prev[0] == "apply_update": hit("H9", i)
            if prev[0] == "timing": hit("H10", i)
        if name == "hint": hint = (kw["first"], kw["n"])
        elif name in ("step_range", "apply_update"): ahead, hint, replaced, uploaded = hint, None, False, False
        elif name == "train_range":
            nb = N // kw["B"]
            ahead, hint, replaced, uploaded = (((kw["first"] // kw["B"] + kw["n_steps"]) % nb) * kw["B"], kw["B"]), None, False, False
        elif name in TRAINING or name == "forget": ahead, hint = None, None
        elif name in REPLACING: replaced = ahead is not None
        elif name == "upload":
            uploaded = ahead is not None
            N = rows_of(kw["which"])
        if name == "step_host":
            f = nxt[0]
            if _is_above(nxt): f = "eval_above"
            if f in H3_FOLLOWERS: hit("H3:" + f, i)
        # H6: three gradient computations in a row by one entry point, of 33 or 40 rows, then 3 or fewer, then 17
        if name in ("step_host", "step_range", "step_indexed"):
            trio = [o for o in ops[:i + 1] if o[0] in TRAINING + ("compute_gradient_range", "weight_gradient")][-3:]
            sizes = [_rows_of(o) for o in trio]
            if len(trio) == 3 and all(o[0] == name for o in trio) and sizes[0] in (33, 40) and sizes[1] <= 3 and sizes[2] == 17:
                hit("H6:" + name, i)
        if name == "train_observed" and prev[0] == "sample" and i >= 2 and ops[i - 2][0] == "train_sampled" and 16 < ops[i - 2][1]["iters"] < 48:
            hit("H7", i)
    return found


def sampler_refills(ops):
    """how many draws of the sequence's samplers refill INSIDE a batch (0 < remaining < B), counted as NNT:143-168 draws"""
    N, remaining, inside = ROWS, ROWS, 0
    for name, kw in ops:
        if name == "upload" and rows_of(kw["which"]) != N:
            N = remaining = rows_of(kw["which"])           # a new sampler for the new size
        draws = {"sample": 1, "train_sampled": kw.get("iters"), "train_observed": kw.get("iters")}.get(name, 0)
        for _ in range(draws):
            B = kw["B"]
            if remaining == 0: remaining = N
            if remaining < B:
                inside += 1
                remaining = N - (B - remaining)
            else:
                remaining -= B
    return inside


# ---- the model ------------------------------------------------------------------------------------------------------------------
def _pad16(n):
    return (n + cc.PAD - 1) // cc.PAD * cc.PAD


class Model:
    """W, V, time, the recorded gradient, the data set and an oracle sampler; `apply(i, op)` returns what the op must return.
    fault: None or one of FAULTS.  reads=False skips the arithmetic of the read ops (a faulty run needs the trajectory only)."""

    def __init__(self, oracle_mod, case, fault=None, reads=True):
        self.o, self.case, self.fault, self.reads = oracle_mod, case, fault, reads
        self.dims, self.inner, self.out_kind, self.last = case["dims"], case["inner"], case["out_kind"], case["last"]
        self.bf16 = case["dtype"] == "bf16"
        self.ref = oracle_mod.OracleNet(self.dims, out_kind=self.out_kind, inner_act=self.inner, last_act=self.last)
        self.ref.set_alloc_per_sample(0)
        self.step, self.mom = case.get("step", cc.STEP), case.get("momentum", cc.MOMENTUM)
        self.W = start_weights(oracle_mod, self.dims, seed=case.get("wseed", 1))
        self.V = np.zeros_like(self.W)
        self.time = self.steps = 0
        self.G = None                      # compute_gradient_range's, waiting for apply_update
        self.exported = None               # a gradient left in the shared buffer by a call that is no step
        self.which = 0
        self.X, self.Y = dataset(case["seed"], 0, self.dims[0], self.dims[-1])
        self.Xh, self.Yh = host_pool(case["seed"], self.dims[0], self.dims[-1])
        self.sampler = oracle_mod.Sampler(len(self.X), seed=SAMPLER_SEED)
        self.each = oracle_mod.Sampler(len(self.X), seed=case.get("each_seed", 2))    # a group member's own sampler
        self.saves = {}
        self.ahead = None                  # dict(key, W, X, Y, replaced, uploaded): the batch with first-layer sums made ahead
        self.hint = None
        self.pending = None                # a host-batch step whose update rides in the next call: dict(G, n, W, V) before it
        self.prev = None                   # (X, Y) of the batch before this one
        self.stale_W = None                # F8: what the bf16 shadow still holds
        self.events = []
        self.Wnew, self.Vnew = replacement_weights(oracle_mod, self.dims), replacement_momentum(oracle_mod, self.dims)

    # -- arithmetic ---------------------------------------------------------------------------------------------------------------
    def _Ws(self, W=None):
        return np_oracle.split(self.W if W is None else W, self.dims)

    def _gradient(self, X, Y, W1=None):
        """sum of the rows' gradients at the current weights; W1: the first-layer sums taken from THESE first-layer weights"""
        if self.bf16:
            if W1 is None:
                return np_oracle.gradient_bf16(self._Ws(), X, Y, self.inner, self.out_kind, self.last)
            W1 = np_oracle.bf16_round(W1)
        Ws = self._Ws()
        if W1 is None and not self.bf16:
            return np_oracle.gradient(Ws, X, Y, self.inner, self.out_kind, self.last)
        q = np_oracle.bf16_round if self.bf16 else (lambda a: a)
        Z = [np.asarray(X, dtype=np.float64)]
        for l, Wl in enumerate(Ws):
            Z.append(q(np_oracle.act(self.inner, Z[-1])) @ (W1 if l == 0 else q(Wl)))
        if self.out_kind == cc.OUT_SOFTMAX_CE:
            e = np.exp(Z[-1] - Z[-1].max(axis=1, keepdims=True))
            D = e / e.sum(axis=1, keepdims=True) - Y
        else:
            D = (np_oracle.act(self.last, Z[-1]) - Y) * np_oracle.act_prime(self.last, Z[-1])
        G = [None] * len(Ws)
        for l in range(len(Ws) - 1, -1, -1):
            G[l] = q(np_oracle.act(self.inner, Z[l])).T @ q(D)
            if l >= 1:
                D = (q(D) @ q(Ws[l]).T) * np_oracle.act_prime(self.inner, Z[l])
        return np.concatenate([g.ravel() for g in G])

    def _update(self, G, n):
        adj = self.step * G / n + self.mom * self.V           # SCE:333
        self.W, self.V = self.W - adj, adj
        self.time += 1; self.steps += 1

    def _event(self, name, i):
        self.events.append((name, i))

    def _train(self, i, X, Y, key=None, host=False):
        n, W1 = len(X), None
        before = (self.W, self.V)
        if key is not None and self.ahead is not None and self.ahead["key"] == key:
            if self.ahead["replaced"]:
                self._event("F1", i)
                if self.fault == "F1": W1 = np_oracle.split(self.ahead["W"], self.dims)[0]
            if self.ahead["uploaded"]:
                self._event("F7", i)
                if self.fault == "F7": X, Y = self.ahead["X"], self.ahead["Y"]
        extra = None
        if self.prev is not None and len(self.prev[0]) > n:
            m = min(len(self.prev[0]), _pad16(n))
            if m > n:
                self._event("F5", i)
                if self.fault == "F5": extra = (self.prev[0][n:m], self.prev[1][n:m])
        add = None
        if self.exported is not None:
            self._event("F4", i)
            if self.fault == "F4": add = self.exported
        self.exported = None
        plain = W1 is None and extra is None and add is None
        if plain and not self.bf16:
            self.ref.set_weights(self.W); self.ref.set_momentum(self.V)
            self.ref.gradient_step(X, Y, self.step, self.mom)
            G = None
            self.W, self.V = self.ref.get_weights(), self.ref.get_momentum()
            self.time += 1; self.steps += 1
        else:
            G = self._gradient(X, Y, W1)
            if extra is not None: G = G + self._gradient(extra[0], extra[1])
            if add is not None: G = G + add
            self._update(G, n)
        self.prev = (X, Y)
        self.stale_W = None
        nxt, self.hint = self.hint, None
        self.ahead = None
        if nxt is not None and not host:
            self._leave_sums(nxt)
        if host:
            self.pending = dict(G=G, n=n, W=before[0], V=before[1])

    def _leave_sums(self, key):
        first, n = key
        self.ahead = dict(key=key, W=self.W, X=self.X[first:first + n], Y=self.Y[first:first + n], replaced=False, uploaded=False)

    def _forward(self, X):
        """(outputs, what the argmax is taken of)"""
        W = self.stale_W if (self.fault == "F8" and self.stale_W is not None) else self.W
        if self.bf16:
            Z, _, out = np_oracle.forward_bf16(self._Ws(W), X, self.inner, self.out_kind, self.last)
            return out, (Z[-1] if self.out_kind == cc.OUT_SOFTMAX_CE else out)
        self.ref.set_weights(W)
        out = self.ref.propagate(X)
        return out, (self.ref.logits(X) if self.out_kind == cc.OUT_SOFTMAX_CE else out)

    def _losses(self, X, Y):
        if self.bf16:
            out = self._forward(X)[0]
            return -(Y * np.log(out)).sum(axis=1) if self.out_kind == cc.OUT_SOFTMAX_CE else (0.5 * (out - Y) ** 2).sum(axis=1)
        self.ref.set_weights(self.W)
        return self.ref.calculate_loss(X, Y)

    def _labels(self, X):
        z = self._forward(X)[1]
        s = np.sort(z, axis=1)
        safe = (s[:, -1] - s[:, -2]) > MARGIN[self.out_kind]
        lab = np.array([self.o.argmax_rule(r) for r in z], dtype=np.int32)      # `>=`: ties go to the highest index (MT:166-168)
        return lab, safe

    # -- one op -------------------------------------------------------------------------------------------------------------------
    def apply(self, i, op):
        name, kw = op
        out = {}
        pend, self.pending = self.pending, None
        if pend is not None and name not in TRAINING:
            self._event("F2", i)
            if self.fault == "F2": self.W, self.V = pend["W"], pend["V"]
        late = pend is not None and name in ("set_weights", "set_momentum", "load")
        if late:
            self._event("F3", i)
            if self.fault == "F3": self.W, self.V = pend["W"], pend["V"]
        rows = lambda: (self.Xh[kw["off"]:kw["off"] + kw["n"]], self.Yh[kw["off"]:kw["off"] + kw["n"]])
        res = lambda: (self.X[kw["first"]:kw["first"] + kw["n"]], self.Y[kw["first"]:kw["first"] + kw["n"]])
        if name == "step_host":
            self._train(i, *rows(), host=True)
        elif name == "step_range":
            self._train(i, *res(), key=(kw["first"], kw["n"]))
        elif name == "step_indexed":
            idx = np.asarray(kw["idx"])
            self._train(i, self.X[idx], self.Y[idx])
        elif name == "train_range":
            B, N = kw["B"], len(self.X)
            for s, r in enumerate(cc.range_batches(N, B, kw["first"], kw["n_steps"])):
                self._train(i, self.X[r:r + B], self.Y[r:r + B], key=(r, B) if s == 0 else None)
            self._leave_sums((cc.range_batches(N, B, kw["first"], kw["n_steps"] + 1)[-1], B))
        elif name in ("train_sampled", "train_observed"):
            vals = []
            for _ in range(kw["iters"]):
                idx = (self.each if kw.get("each") else self.sampler).sample(kw["B"])
                self._train(i, self.X[idx], self.Y[idx])
                if name == "train_observed" and self.reads:
                    vals.append(self._losses(self.X[:kw["V"]], self.Y[:kw["V"]]).sum() / kw["V"])
            if name == "train_observed": out["val"] = np.array(vals)
        elif name == "sample":
            out["idx"] = self.sampler.sample(kw["B"])
        elif name == "compute_gradient_range":
            X, Y = res()
            self.G = self.exported = self._gradient(X, Y)
            self.prev = (X, Y)
            self.ahead = None if self.ahead is None or self.ahead["key"] != (kw["first"], kw["n"]) else self.ahead
        elif name == "apply_update":
            self._update(self.G, kw["B"])                       # SCE:324-344 with batchSize = B_global
            self.exported, self.stale_W = None, None
            nxt, self.hint, self.ahead = self.hint, None, None
            if nxt is not None: self._leave_sums(nxt)
        elif name == "hint":
            self.hint = (kw["first"], kw["n"])
        elif name == "weight_gradient":
            X, Y = rows()
            self.exported = self._gradient(X, Y)
            self.prev = (X, Y)
            out["grad"] = self.exported
        elif name == "set_weights":
            self.stale_W = self.W
            self.W = self.Wnew.copy()
            if self.ahead is not None: self.ahead["replaced"] = True
        elif name == "set_momentum":
            self.V = self.Vnew.copy()
        elif name == "save":
            self.saves[kw["slot"]] = (self.W.copy(), self.V.copy(), self.time)
        elif name == "load":
            W, V, t = self.saves[kw["slot"]]
            self.stale_W = self.W
            self.W, self.time = W.copy(), t
            if self.fault != "F6": self.V = V.copy()
            self._event("F6", i)
            if self.ahead is not None: self.ahead["replaced"] = True
        elif name == "upload":
            self.which = kw["which"]
            old = len(self.X)
            self.X, self.Y = dataset(self.case["seed"], self.which, self.dims[0], self.dims[-1])
            if len(self.X) != old: self.sampler = self.o.Sampler(len(self.X), seed=SAMPLER_SEED)
            if self.ahead is not None: self.ahead["uploaded"] = True
            self.hint = None
        elif name == "forget":
            self.ahead, self.hint = None, None
        elif name == "advance_time":
            self.time += kw["n"]
        elif name in ("specialize", "timing", "synchronize", "refused"):
            pass
        elif self.reads or (name == "propagate" and self.fault == "F8"):
            if name == "propagate":
                out["out"] = self._forward(rows()[0])[0]
            elif name == "loss":
                out["loss"] = self._losses(*rows())
            elif name == "argmax":
                out["labels"], out["safe"] = self._labels(rows()[0])
            elif name == "loss_range":
                out["loss"] = self._losses(*res())
            elif name in ("argmax_range", "labels", "confusion"):
                out["labels"], out["safe"] = self._labels(res()[0])
            elif name in ("count_hits", "evaluate"):
                X, Y = res()
                lab, safe = self._labels(X)
                want = np.array([np.flatnonzero(y == 1)[-1] for y in Y])       # the LAST index whose expected value is 1 (MT:186-188)
                out["hits"], out["unsafe"], out["safe"] = int((lab == want).sum()), int((~safe).sum()), safe
                if name == "evaluate": out["loss_sum"] = float(self._losses(X, Y).sum())
            elif name == "get_weights": out["W"] = self.W.copy()
            elif name == "get_momentum": out["V"] = self.V.copy()
        if name == "propagate" and self.stale_W is not None: self._event("F8", i)
        if late and self.fault == "F3":                         # ... and the pending update lands on what the call has just written
            adj = self.step * pend["G"] / pend["n"] + self.mom * self.V
            self.W, self.V = self.W - adj, adj
        out["time"], out["steps"] = self.time, self.steps
        return out


def is_checkpoint(i, ops):
    """weights and momentum are compared behind op i: every 8 ops, at the end, and in front of a load_checkpoint (which wipes both)
    unless a host-batch step's update is pending there (the read would apply it)"""
    return i % CHECK_EVERY == CHECK_EVERY - 1 or i == len(ops) - 1 or (ops[i + 1][0] == "load" and ops[i][0] != "step_host")


def run_model(oracle_mod, case, n_ops=None):
    """The correct model over the first n_ops ops: per-op results (with W and V at every checkpoint), the hazard events, and for
    every kind of event the model state in front of the op where it first fired (what a faulty run starts from)."""
    ops = case["ops"][:n_ops]
    m = Model(oracle_mod, case)
    results, snaps, seen = [], {}, set()
    for i, op in enumerate(ops):
        snap = _snapshot(m)
        n_ev = len(m.events)
        r = m.apply(i, op)
        for name, _ in m.events[n_ev:]:
            if name not in seen:
                seen.add(name); snaps[name] = (i, snap)
        if is_checkpoint(i, ops):
            r["W"], r["V"] = m.W.copy(), m.V.copy()
        results.append(r)
    return results, m.events, snaps


_STATE = ("W", "V", "time", "steps", "G", "exported", "which", "X", "Y", "saves", "ahead", "hint", "pending", "prev", "stale_W")


def _snapshot(m):
    s = {k: getattr(m, k) for k in _STATE}                      # (arrays are replaced, never written in place)
    s["saves"] = dict(m.saves)
    s["ahead"] = None if m.ahead is None else dict(m.ahead)
    return s


def fault_factor(oracle_mod, case, fault, results, snaps):
    """How far (in budgets) the model with `fault` is from the correct one at the first checkpoint at or behind the op where the
    fault's hazard first occurs; None when the sequence does not contain the hazard.  F8 is looked for where the test looks: at the
    first propagate behind the replacement, against the 5e-3 of the bf16 outputs."""
    if fault not in snaps or (fault == "F8") != (case["dtype"] == "bf16"):
        return None
    i0, snap = snaps[fault]
    m = Model(oracle_mod, case, fault=fault, reads=False)
    for k, v in snap.items():
        setattr(m, k, v)
    m.saves = dict(snap["saves"]); m.ahead = None if snap["ahead"] is None else dict(snap["ahead"])
    ops = case["ops"]
    if m.pending is not None and m.pending["G"] is None:       # the step's gradient, from the update it made (SCE:333)
        m.pending = dict(m.pending, G=(m.V - cc.MOMENTUM * m.pending["V"]) * m.pending["n"] / cc.STEP)
    # (the sampler is not part of the snapshot: none of the faults' hazards lies in front of a sampled loop's draws unless replayed)
    m.sampler = _sampler_at(oracle_mod, case, i0)
    for i in range(i0, len(ops)):
        r = m.apply(i, ops[i])
        if fault == "F8":
            if ops[i][0] == "propagate":
                ok = Model(oracle_mod, case, reads=True)
                for k, v in _snapshot(m).items(): setattr(ok, k, v)
                want = ok._forward(m.Xh[ops[i][1]["off"]:ops[i][1]["off"] + ops[i][1]["n"]])[0]
                return float(np.abs(r["out"] - want).max() / BF16_OUT)
            if ops[i][0] in TRAINING: return 0.0
            continue
        budget = W_ATOL * max(results[i]["steps"], 1)
        if ops[i][0] == "get_weights":                           # (a read is a check as well: the FIRST check counts, whatever it shows)
            return float(np.abs(m.W - results[i]["W"]).max() / budget)
        if ops[i][0] == "get_momentum":
            return float(np.abs(m.V - results[i]["V"]).max() / budget)
        if is_checkpoint(i, ops):
            return float(max(np.abs(m.W - results[i]["W"]).max(), np.abs(m.V - results[i]["V"]).max()) / budget)
    return 0.0


def _sampler_at(oracle_mod, case, i0):
    """the oracle sampler as the first i0 ops leave it"""
    N, s = ROWS, oracle_mod.Sampler(ROWS, seed=SAMPLER_SEED)
    for name, kw in case["ops"][:i0]:
        if name == "upload" and rows_of(kw["which"]) != N:
            N = rows_of(kw["which"]); s = oracle_mod.Sampler(N, seed=SAMPLER_SEED)
        for _ in range({"sample": 1, "train_sampled": kw.get("iters"), "train_observed": kw.get("iters")}.get(name, 0)):
            s.sample(kw["B"])
    return s


# ---- groups ---------------------------------------------------------------------------------------------------------------------
# name, dims, inner, out_kind, last, dtype, K: two f32 two-launch shapes (K = 2, runtime shape; K = 3, prebuilt), a bf16 one, and
# K = 16 of a shape OFF the grouped path (middle4_kernel is its row kernel: launches_per_step == 0, the members stepped in turn)
GROUPS = [
    ("g-f32-k2", [65, 20, 12, 5], LEAKY, cc.OUT_SOFTMAX_CE, IDENT, "f32", 2),
    ("g-f32-prebuilt-k3", [784, 100, 50, 10], LEAKY, cc.OUT_SOFTMAX_CE, IDENT, "f32", 3),
    ("g-bf16-k3",) + _chain(18) + ("bf16", 3),
    ("g-f32-off-path-k16",) + _chain(19) + ("f32", 16),
]
N_GROUP = len(GROUPS) * SEEDS_PER_NET
GROUP_OPS = ("g_train_range", "g_train_sampled", "g_train_observed", "g_evaluate", "g_confusion", "g_ensemble", "g_upload", "member")
PAIRS = ("sums-then-member-k", "sums-then-member-0", "sized-then-uniform", "evaluation-between-loops")


def group_case(i):
    name, dims, inner, out_kind, last, dtype, K = GROUPS[i // SEEDS_PER_NET]
    seed = 9500 + i
    return dict(id="%s-%d" % (name, i % SEEDS_PER_NET), net=name, dims=list(dims), inner=inner, out_kind=out_kind, last=last, dtype=dtype,
                seed=seed, K=K, wseeds=[k + 1 for k in range(K)], each_seeds=[11 + k for k in range(K)],
                steps=[cc.STEP * (1.0 - 0.03 * k) for k in range(K)], momenta=[cc.MOMENTUM - 0.01 * k for k in range(K)],
                ops=draw_group_ops(seed, K))


def member_case(case, k):
    """member k of a group case as the lone net that makes its calls"""
    return dict(case, id="%s[%d]" % (case["id"], k), wseed=case["wseeds"][k], each_seed=case["each_seeds"][k], step=case["steps"][k],
                momentum=case["momenta"][k], ops=[member_op(op, k) for op in case["ops"]])


def member_op(op, k):
    """the call a lone net makes in member k's place (None: none)"""
    name, kw = op
    if name == "member":
        return kw["op"] if kw["k"] == k and kw["op"][0] != "refused" else None
    if name == "g_train_range": return ("train_range", kw)
    if name == "g_train_sampled":
        return ("train_sampled", dict(iters=kw["iters"], B=kw["B"][k] if kw["mode"] == "sizes" else kw["B"], each=kw["mode"] != "shared"))
    if name == "g_train_observed": return ("train_observed", dict(iters=kw["iters"], B=kw["B"], V=kw["V"]))
    if name == "g_evaluate": return ("evaluate", kw)
    if name == "g_confusion": return ("confusion", kw)
    if name == "g_upload": return ("upload", kw)
    return None                                                  # g_ensemble: the group's alone


def draw_group_ops(seed, K):
    """About 35 calls on a group: every grouped call form, members 0, a middle one and the last stepped, written, restored and
    read alone, and the planted PAIRS (group_pairs finds them)."""
    d = _Draw(seed)
    mid, last = K // 2, K - 1
    member = lambda k, name, **kw: d.add("member", k=k, op=(name, kw))
    d.add("g_train_range", first=0, B=17, n_steps=3)
    for k in sorted({0, mid, last}):
        member(k, "save", slot=0)

    def alone(k, r):
        n = d.pick(BATCHES)
        if r == 0: member(k, "step_range", first=d.first(n), n=n)
        elif r == 1: member(k, "step_host", **d.host(n))
        else: member(k, "set_weights")

    def sums_member(k, r):
        call, nxt = d.range_call()
        d.add("g_train_range", **call); alone(k, r); d.add("g_train_range", first=nxt[0], B=nxt[1], n_steps=int(d.rng.integers(1, 4)))

    def sized(_):
        d.add("g_train_sampled", mode="sizes", iters=int(d.rng.integers(2, 6)), B=[d.pick(BATCHES) for _ in range(K)])
        d.add("g_train_sampled", mode="shared", iters=int(d.rng.integers(1, 5)), B=d.pick((16, 33, 40)))

    def each(_):
        d.add("g_train_sampled", mode="each", iters=int(d.rng.integers(2, 5)), B=d.pick((17, 33)))
        member(mid, "refused", kind="upload")
        d.add("g_train_observed", iters=int(d.rng.integers(2, 4)), B=d.pick((5, 17, 40)), V=d.pick((7, ROWS // 100 + 1, 57)))

    def evaluation(_):
        call, nxt = d.range_call(2)
        d.add("g_train_range", **call)
        _add(d, ("g_" + d.pick(("evaluate", "confusion")), d.above()[1]))
        d.add("g_train_range", first=nxt[0], B=nxt[1], n_steps=2)

    def restore(_):
        k = d.pick((0, mid, last))
        member(k, "step_host", **d.host(d.pick(BATCHES))); member(k, "load", slot=0); member(k, "propagate", **d.host(5))
        _add(d, ("member", dict(k=k, op=("evaluate", d.above()[1]))))
        d.add("g_train_sampled", mode="shared", iters=2, B=16)

    def reads(_):
        n = d.pick((5, 17, 40))
        d.add("g_ensemble", first=d.first(n), n=n)
        d.add("g_evaluate", **d.below()[1]); d.add("g_confusion", **d.above()[1])
        member(last, "propagate", **d.host(16)); member(0, "evaluate", **d.above()[1])

    def upload(_):
        call, nxt = d.range_call()
        d.add("g_train_range", **call); d.add("g_upload", which=1); d.add("g_train_range", first=nxt[0], B=nxt[1], n_steps=1)

    r0 = int(d.rng.integers(0, 3))
    blocks = [lambda: sums_member(last, r0 % 2), lambda: sums_member(mid if mid else last, 2), lambda: sums_member(0, r0), lambda: sized(0), lambda: each(0),
              lambda: evaluation(0), lambda: restore(0), lambda: reads(0), lambda: upload(0)]
    for i in d.rng.permutation(len(blocks)):
        blocks[int(i)]()
    return d.ops


def group_pairs(ops):
    """{pair: [op indices]} of the planted PAIRS in a group sequence"""
    found, ahead = {}, None
    def hit(h, i): found.setdefault(h, []).append(i)
    for i, (name, kw) in enumerate(ops):
        prev = ops[i - 1] if i else ("", {})
        if name == "g_train_range":
            if ahead == (kw["first"], kw["B"]) and prev[0] == "member" and prev[1]["op"][0] in ("step_range", "step_host", "set_weights"):
                hit("sums-then-member-0" if prev[1]["k"] == 0 else "sums-then-member-k", i)
            if ahead == (kw["first"], kw["B"]) and prev[0] in ("g_evaluate", "g_confusion"):
                hit("evaluation-between-loops", i)
            nb = ROWS // kw["B"]
            ahead = (((kw["first"] // kw["B"] + kw["n_steps"]) % nb) * kw["B"], kw["B"])
        elif name in ("g_train_sampled", "g_train_observed"):
            if prev[0] == "g_train_sampled" and prev[1]["mode"] == "sizes" and kw.get("mode") != "sizes": hit("sized-then-uniform", i)
            ahead = None
        elif name == "g_upload":
            ahead = None
    return found
