"""The SECOND draw of call sequences: the calls merged since tests/sequence_cases.py froze its vocabulary, planted between the steps
of a chain (tests/test_sequence_cases_cpu.py pins the draw and the power of the budgets; tests/test_call_sequences_gpu.py runs it).
No GPU and no product code.  Model, _Draw, dataset and host_pool are sequence_cases'; its draws stay what they were (the CPU test
pins a digest of every one of them).

New ops, beside the old vocabulary:
  reading   input_gradient (host rows)  input_gradient_range  get_targets  propagate_set  evaluate_set (kind = evaluate | confusion |
            labels, either set, n below and above max_batch)  fgsm_range  evaluate_fgsm
  writing   upload_held_out (23, 57 or 101 rows: 101 is the training set's count)  set_targets  distill (teacher = self | other |
            group, keep in 0, 0.25, 1)
  training  train_held_out  train_fgsm
  refused   refused2 (kind = no_held_out | fgsm | distill_dims | targets_rows), each behind a pending host-batch update
  teacher   (op): a call of the old vocabulary on the SECOND handle T, the `other` teacher, which has a chain of its own
The perturbing ops come in two kinds (the sign of a tiny g is the implementer's): clip-only -- eps = 0, clip (0.25, 0.75), every
element decided, rows compared in full; train_fgsm and evaluate_fgsm always are -- and signed -- eps = 0.1, clip (0, 1), fgsm_range
only, compared on adversarial_cases.decided elements, whose complement tests/test_sequence_cases_cpu.py holds below UNDECIDED_CAP at
every such op.  Nets whose inner activation the adversarial calls refuse (tanh: f32-middle4; sigmoid: f32-general, bf16-middle4)
get refused2(kind = fgsm) where the others get a perturbing op, and input_gradient_range in the hazards that need a gradient-only call.

Nets: sequence_cases.NETS and a ninth, f32-general-leaky -- GeneralNeuralNet, leaky inner, sigmoid output, 556-105-12 -- which runs
the adversarial calls and input_gradient on the General output head.  Two sequences per net.

Planted (hazards2): H11 a host-batch step with each new call right behind it; H12 a gradient left behind by a gradient-only call
(last block 33 or 40 rows) in front of a step of 3 to 5 rows, and between compute_gradient_range and apply_update; H13 a gradient-only
call on training rows between a step and the batch it prepared (a: another last block, b: that very batch, loop: behind train_range);
H14 a perturbing call on held-out rows, a host-batch step of its last block's size, a propagate; H15 targets rewritten between a
step and the batch it prepared, and between two equal evaluations; H16 the teacher T hinted, stepped, used, stepped on the hinted
batch, read; T and the student with an update pending in front of a distill; H17 the held-out set uploaded and evaluated inside a
chain, and with the training set's row count; H18 the keep-best loop across the sampler's first chunk, then sample, then
train_sampled; H19 train_fgsm behind a hinted step and in front of a step on the batch prepared before it.

Faults (Model2, beside F1 .. F8 of sequence_cases.Model):
  F9  a new read op answers from the weights before the pending update     F13 the step on a batch prepared ahead uses the targets
  F10 the gradient a gradient-only call left is added to the next step's       from before the rewrite
  F11 the step behind a gradient-only call takes first-layer sums of that  F14 after a distillation the teacher's next step and
      call's last block                                                        loss_range run on the student's rows
  F12 the adversarial step takes first-layer sums of the unperturbed rows; F15 an evaluation of the held-out set reads training rows
      a host-batch step behind a perturbing call those of the perturbed    F16 the best weights are those one step later
      staging rows                                                         F17 the momentum train_held_out / train_fgsm leaves is one
                                                                               iteration old
Least distance of a faulty model from the correct one at the first check behind the hazard, in budgets, over the 18 sequences
(tests/test_sequence_cases_cpu.py asserts >= 2 for every sequence and prints them): F9 3.11, F10 47.6, F11 29.8, F12 10.9, F13 13.7,
F14 1070, F15 18.5, F16 23.9, F17 6.47 (FAULT_FACTORS_FOUND2); one pair is beyond the f32 budgets (TWIN_ONLY).  A check is a
checkpoint, a get_weights / get_momentum, the teacher's loss_range or get_weights (F14), or -- F9, F15, F16 -- the read op's own
result.  What moved the draw there: H13 is planted first, while the budget of seven steps is small, with a get_weights behind its
step (stale sums of a narrow first layer: 0.9 budgets forty steps later); the evaluations behind a pending update read 1 or 3 rows
(over 16 and more the rows' changes cancel in the mean loss: 0.07 to 0.8); a get_momentum stands behind train_fgsm and the short
train_held_out; hit counts are measured like every other budget (|difference| / (unsafe rows + 0.5): above 1 exactly when the device
test fails); sequence 17 has a draw seed of its own (DRAW_SEEDS).  F9 is measured where the first new read of a sequence meets a
pending update; over EVERY such read the least is 0.2 (an evaluate_fgsm of clipped rows on the General head, whose loss one step
barely moves) -- those results are held to the twin's bit for bit as well.

Length: about 125 calls and 80 to 110 steps a lone sequence (H11 alone has eighteen followers), 27 calls a group sequence; on the
MI355X a lone case takes at most 1.3 s, a group case at most 1.3 s."""
import functools
import hashlib

import numpy as np

from tests import adversarial_cases as ac
from tests import chain_cases as cc
from tests import input_gradient_cases as igc
from tests import np_oracle
from tests import sequence_cases as sq
from tests import soft_target_cases as stc

MAX_BATCH, BATCHES, ROWS, HOST_ROWS = sq.MAX_BATCH, sq.BATCHES, sq.ROWS, sq.HOST_ROWS
SEEDS_PER_NET = 2
NETS = sq.NETS + [("f32-general-leaky",) + (sq._chain(14)[0], sq.LEAKY, cc.OUT_ACT_LOSS, sq.SIGMOID, "f32")]
N_LONE = len(NETS) * SEEDS_PER_NET
HELD_SIZES = (23, 57, 101)
CLIP_ONLY = dict(eps=0.0, clip=(0.25, 0.75))
SIGNED = dict(eps=0.1, clip=(0.0, 1.0))
KEEPS = (0.0, 0.25, 1.0)
TEACHER_HIDDEN = 24                # the `other` teacher: dims[0]-24-dims[-1]
GROUP_SEEDS = (5, 6)               # the `group` teacher: two nets of the student's dims, never trained
FAULTS = ("F9", "F10", "F11", "F12", "F13", "F14", "F15", "F16", "F17")
FAULT_FACTORS_FOUND2 = {"F9": 3.11, "F10": 47.6, "F11": 29.8, "F12": 10.9, "F13": 13.7, "F14": 1070.0, "F15": 18.5, "F16": 23.9, "F17": 6.47}
# (net, fault) pairs the f32 budgets cannot resolve, with the reason; the device test holds these sequences to the twin bit for bit
TWIN_ONLY = {("bf16-middle4", "F11"): "573-14-..: a sigmoid inner activation maps the rows (half zeros, else U[0, 1)) into [0.5, 0.73], so "
                                      "first-layer sums of ANOTHER batch differ by little: 0.37 and 0.77 budgets"}
DATA_SEEDS = {}                    # sequence -> the seed of its data where its own broke a condition on the draw
DRAW_SEEDS = {17: 10017}            # sequence -> the seed of its draw where its own left a fault within 2 budgets (F9: 0.203)
FGSM_INNER = (sq.LEAKY, sq.RELU, sq.IDENT)
GRAD_ONLY = ("input_gradient_range", "fgsm_range", "evaluate_fgsm")
NEW_READS = ("input_gradient", "input_gradient_range", "get_targets", "propagate_set", "evaluate_set", "fgsm_range", "evaluate_fgsm")
NEW_WRITES = ("upload_held_out", "set_targets", "distill")
NEW_TRAINING = ("train_held_out", "train_fgsm")
NEW_OPS = NEW_READS + NEW_WRITES + NEW_TRAINING + ("refused2", "teacher")
REFUSALS = ("no_held_out", "fgsm", "distill_dims", "targets_rows")
# the reads whose answer depends on the weights (F9 is looked for in their own result)
F9_READS = ("input_gradient", "input_gradient_range", "propagate_set", "evaluate_set", "evaluate_fgsm")
H11_FOLLOWERS = NEW_READS + ("upload_held_out", "set_targets", "distill:self", "distill:other", "distill:group", "distill:teacher",
                             "train_held_out", "train_fgsm") + tuple("refused2:" + k for k in REFUSALS if k != "fgsm")
# (refused2(kind = fgsm) stands where fgsm_range, evaluate_fgsm and train_fgsm stand on the nets that run them)


def digest(ops):
    """of an op list: what tests/test_sequence_cases_cpu.py pins the old draws with"""
    return hashlib.sha256(repr(ops).encode()).hexdigest()[:16]


def fgsm_ok(inner):
    return inner in FGSM_INNER


def lone_case(i):
    """Sequence i of the 18: net i // 2, draw seed i % 2."""
    name, dims, inner, out_kind, last, dtype = NETS[i // SEEDS_PER_NET]
    seed = DRAW_SEEDS.get(i, 9700 + i)
    return dict(id="%s-new-%d" % (name, i % SEEDS_PER_NET), net=name, dims=list(dims), inner=inner, out_kind=out_kind, last=last, dtype=dtype,
                seed=DATA_SEEDS.get(i, seed), draw_seed=seed, ops=draw_ops(seed, fgsm_ok(inner)))


def teacher_case(case):
    """the second handle T of a sequence: other hidden widths, rows and start weights of its own"""
    return dict(case, id=case["id"] + "[T]", dims=[case["dims"][0], TEACHER_HIDDEN, case["dims"][-1]], seed=case["seed"] + 1000, wseed=4, ops=[])


@functools.lru_cache(maxsize=64)
def held_set(seed, size, d_in, d_out):
    return sq._rows(31 * seed + 500 + size, size, d_in, d_out)


@functools.lru_cache(maxsize=256)
def target_rows(seed, tseed, n, d_out):
    """set_targets' rows, f32-exact: soft rows that sum to 1, four in ten of them one-hot rows of a drawn class"""
    rng = np.random.default_rng(77 * seed + tseed)
    t = 2.0 * rng.standard_normal((n, d_out))
    e = np.exp(t - t.max(axis=1, keepdims=True))
    Y = e / e.sum(axis=1, keepdims=True)
    hot = rng.random(n) < 0.4
    Y[hot] = np.eye(d_out)[rng.integers(0, d_out, int(hot.sum()))]
    Y = Y.astype(np.float32).astype(np.float64)
    Y.setflags(write=False)
    return Y


def blocks_of(first, n):
    """the (first, rows) blocks a range call walks"""
    return [(first + o, min(MAX_BATCH, n - o)) for o in range(0, n, MAX_BATCH)]


def clip_rows(X, signed_g=None):
    """the perturbed rows: clip-only, or signed with the gradient given"""
    if signed_g is None:
        return ac.perturb(X, np.zeros_like(X), CLIP_ONLY["eps"], CLIP_ONLY["clip"])
    return ac.perturb(X, signed_g, SIGNED["eps"], SIGNED["clip"])


# ---- the draw -------------------------------------------------------------------------------------------------------------------
class _Draw2(sq._Draw):
    def __init__(self, seed, fgsm):
        super().__init__(seed)
        self.fgsm, self.held, self.tseed, self.flip = fgsm, 0, 0, 0
        self.kinds = [GRAD_ONLY[int(i)] for i in self.rng.permutation(3)]
        self.sets = ["evaluate", "confusion", "labels"]

    def grad_kind(self, allowed=GRAD_ONLY):
        """the gradient-only range calls in turn (a net without the adversarial calls: input_gradient_range)"""
        if not self.fgsm:
            return "input_gradient_range"
        while True:
            self.kinds.append(self.kinds.pop(0))
            if self.kinds[-1] in allowed:
                return self.kinds[-1]

    def set_kind(self):
        self.sets.append(self.sets.pop(0))
        return self.sets[-1]

    def grad_only(self, first, n, held=False, allowed=GRAD_ONLY):
        kind = self.grad_kind(allowed)
        if kind == "input_gradient_range":
            self.add(kind, first=first, n=n)
        elif kind == "fgsm_range":
            self.flip ^= 1
            self.add(kind, first=first, n=n, held=held, signed=bool(self.flip))
        else:
            self.add(kind, first=first, n=n, held=held)

    def ending_at(self, f_last, n_last):
        """a range whose LAST block is (f_last, n_last)"""
        k = int(self.rng.integers(0, 2)) if f_last >= MAX_BATCH else 0
        return f_last - k * MAX_BATCH, k * MAX_BATCH + n_last

    def hold(self, least):
        """a held-out set of at least `least` rows"""
        if self.held < least:
            self.held = self.pick([s for s in HELD_SIZES if s >= least])
            self.add("upload_held_out", size=self.held)

    def targets(self, first, n):
        self.tseed += 1
        self.add("set_targets", first=first, n=n, tseed=self.tseed)

    def teacher(self, name, **kw):
        self.add("teacher", op=(name, kw))

    def eval_set(self, held, above, kind=None):
        N = self.held if held else self.N
        n = int(self.rng.integers(MAX_BATCH + 1, N + 1)) if above else self.pick([b for b in BATCHES if b <= N])
        self.add("evaluate_set", kind=kind or self.set_kind(), held=held, first=int(self.rng.integers(0, N - n + 1)), n=n)

    def filler2(self, r):
        n = self.pick(BATCHES)
        if r == 0: self.add("input_gradient", **self.host(n))
        elif r == 1: self.add("get_targets", first=self.first(n), n=n, held=False)
        elif r == 2:
            self.hold(23); self.add("propagate_set", first=0, n=self.held, held=True)
        elif r == 3: self.add("propagate_set", first=self.first(n), n=n, held=False)
        elif r == 4:
            self.hold(57); self.eval_set(True, True)
        elif r == 5:
            self.hold(23); self.eval_set(True, False)
        elif r == 6: self.eval_set(False, True)
        elif r == 7:
            self.hold(23); self.add("get_targets", first=0, n=self.held, held=True)
        else: self.add("forget")


N_FILLERS = 9


def _follower(d, f):
    """H11: a host-batch step, `f` right behind it (the update is pending when it arrives)"""
    n = d.pick(BATCHES)
    if f in ("train_held_out", "evaluate_set"): d.hold(23)
    if f == "distill:teacher":
        d.teacher("step_host", **d.host(n))
    else:
        d.add("step_host", **d.host(n))
    m = d.pick(BATCHES)
    if f == "input_gradient": d.add(f, **d.host(m))
    elif f == "input_gradient_range": d.add(f, first=d.first(m), n=m)
    elif f == "get_targets": d.add(f, first=d.first(m), n=m, held=False)
    elif f == "propagate_set": d.add(f, first=d.first(m), n=m, held=False)
    elif f == "evaluate_set":                                  # (few rows: over many the rows' changes cancel in the mean)
        held = bool(d.rng.integers(0, 2)); m = d.pick((1, 3))
        d.add(f, kind="evaluate", held=held, first=int(d.rng.integers(0, (d.held if held else d.N) - m + 1)), n=m)
    elif f in ("fgsm_range", "evaluate_fgsm", "train_fgsm") and not d.fgsm: d.add("refused2", kind="fgsm", call=f)
    elif f == "fgsm_range": d.add(f, first=d.first(m), n=m, held=False, signed=True)
    elif f == "evaluate_fgsm":
        m = d.pick((1, 3)); d.add(f, first=d.first(m), n=m, held=False)
    elif f == "train_fgsm": d.add(f, iters=int(d.rng.integers(3, 6)), B=d.pick((15, 17)))
    elif f == "upload_held_out":
        d.held = d.pick(HELD_SIZES); d.add(f, size=d.held)
    elif f == "set_targets": d.targets(d.first(m), m)
    elif f.startswith("distill:"):
        who = f.split(":")[1]
        d.add("distill", teacher="other" if who == "teacher" else who, keep=d.pick(KEEPS), first=d.first(m), n=m)
        if who == "teacher": d.teacher("get_weights")
    elif f == "train_held_out":
        d.add(f, iters=int(d.rng.integers(4, 7)), B=d.pick((5, 16, 33)), every=1, held_rows=d.pick((7, d.held)), rule="hits")
    elif f.startswith("refused2:"):
        d.add("refused2", kind=f.split(":")[1], call="")
    if f in ("train_held_out", "train_fgsm"): d.add("get_momentum")


def _blocks2():
    def h12(d):
        n, m = d.pick((33, 40)), d.pick((3, 4, 5))
        f = int(d.rng.integers(0, d.N - n + 1))
        d.grad_only(*d.ending_at(f, n)); d.add("step_range", first=d.first(m), n=m); d.add("get_weights")
        n = d.pick((33, 40)); f = int(d.rng.integers(0, d.N - n + 1)); B = d.pick(BATCHES)
        d.add("compute_gradient_range", first=d.first(B), n=B); d.grad_only(*d.ending_at(f, n)); d.add("apply_update", B=n); d.add("get_momentum")

    def h13(d):
        for variant in ("a", "b"):
            B = d.pick((15, 16, 17, 33))
            fb = d.first(B)
            fa = fb if variant == "b" else (fb + B) % (d.N - B + 1)
            d.add("hint", first=fb, n=B); d.add("step_range", first=d.first(5), n=5)
            d.grad_only(*d.ending_at(fa, B), allowed=("input_gradient_range", "fgsm_range"))
            d.add("step_range", first=fb, n=B)
            if variant == "a": d.add("get_weights")            # (stale sums of a narrow first layer fade within a few steps)
        call, nxt = d.range_call()
        d.add("train_range", **call)
        d.grad_only(*d.ending_at(nxt[0] if d.rng.random() < 0.5 else call["first"], nxt[1]), allowed=("input_gradient_range", "fgsm_range"))
        d.add("step_range", first=nxt[0], n=nxt[1])

    def h14(d):
        if not d.fgsm:
            d.add("step_host", **d.host(17)); d.add("refused2", kind="fgsm", call="evaluate_fgsm"); d.add("propagate", **d.host(17))
            return
        d.held = 57; d.add("upload_held_out", size=57)
        d.grad_only(0, 57, held=True, allowed=("fgsm_range", "evaluate_fgsm")); d.add("step_host", **d.host(17)); d.add("propagate", **d.host(17))
        d.grad_only(*d.pick(((0, 33), (17, 40))), held=True, allowed=("fgsm_range", "evaluate_fgsm")); d.add("propagate", **d.host(d.pick((33, 40))))

    def h15(d):
        for how in ("set_targets", "distill", "beside"):
            B = d.pick((15, 16, 17))
            fb = int(d.rng.integers(0, d.N - 2 * B + 1))
            d.add("hint", first=fb, n=B); d.add("step_range", first=d.first(4), n=4)
            if how == "set_targets": d.targets(max(fb - 3, 0), B + 3)
            elif how == "distill": d.add("distill", teacher="self", keep=0.25, first=fb, n=B)
            else: d.targets(fb + B, B)
            d.add("step_range", first=fb, n=B)
        n = int(d.rng.integers(MAX_BATCH + 1, d.N + 1)); f = int(d.rng.integers(0, d.N - n + 1))
        d.add("evaluate_set", kind="evaluate", held=False, first=f, n=n); d.targets(f + 5, 30)
        d.add("evaluate_set", kind="evaluate", held=False, first=f, n=n)

    def h16(d):
        B = d.pick((15, 16, 17, 33)); fb = int(d.rng.integers(0, ROWS - B + 1))
        d.teacher("hint", first=fb, n=B); d.teacher("step_range", first=int(d.rng.integers(0, ROWS - 16)), n=16)
        d.add("distill", teacher="other", keep=d.pick((0.0, 0.25)), first=0, n=d.N)
        d.teacher("step_range", first=fb, n=B); d.teacher("loss_range", first=fb, n=B); d.teacher("get_weights")
        fs = d.first(B)
        d.add("hint", first=fs, n=B); d.add("distill", teacher="self", keep=0.0, first=d.first(33), n=33)
        d.add("step_range", first=d.first(3), n=3); d.add("step_range", first=fs, n=B)

    def h17(d):
        call, nxt = d.range_call(2)
        d.held = d.pick((57, 101))
        d.add("train_range", **call); d.add("upload_held_out", size=d.held); d.add("train_range", first=nxt[0], B=nxt[1], n_steps=2)
        call, nxt = d.range_call(2)
        d.add("train_range", **call); d.eval_set(True, True); d.add("train_range", first=nxt[0], B=nxt[1], n_steps=1)
        d.held = 101; d.add("upload_held_out", size=101)
        d.add("upload", which=1 - d.which); d.which = 1 - d.which
        d.add("evaluate_set", kind="evaluate", held=True, first=0, n=101); d.add("evaluate_set", kind="evaluate", held=False, first=0, n=101)

    def h18(d):
        d.hold(57)
        every, rule = d.pick((3, 7)), d.pick(("loss", "hits"))
        d.add("train_held_out", iters=int(d.rng.integers(17, 21)), B=d.pick((15, 17)), every=every, held_rows=d.pick((7, 23)), rule=rule)
        d.add("sample", B=d.pick(BATCHES)); d.add("train_sampled", iters=int(d.rng.integers(1, 4)), B=d.pick((5, 16, 33)))
        d.add("train_held_out", iters=int(d.rng.integers(3, 6)), B=d.pick((4, 33)), every=1, held_rows=d.held, rule="hits" if rule == "loss" else "loss")

    def h19(d):
        B = d.pick((15, 16, 17)); fb = d.first(B)
        if not d.fgsm:
            d.add("hint", first=fb, n=B); d.add("step_range", first=d.first(5), n=5); d.add("step_host", **d.host(5))
            d.add("refused2", kind="fgsm", call="train_fgsm"); d.add("step_range", first=fb, n=B)
            return
        d.add("hint", first=fb, n=B); d.add("step_range", first=d.first(5), n=5)
        d.add("train_fgsm", iters=int(d.rng.integers(17, 21)), B=d.pick((15, 17))); d.add("get_momentum")
        d.add("hint", first=fb, n=B); d.add("step_range", first=d.first(5), n=5)
        d.add("train_fgsm", iters=int(d.rng.integers(3, 6)), B=d.pick((15, 17))); d.add("step_range", first=fb, n=B)

    followers = [lambda d, f=f: _follower(d, f) for f in H11_FOLLOWERS if f != "refused2:no_held_out"]
    return [h12, h13, h14, h15, h16, h17, h18, h19] + followers


def draw_ops(seed, fgsm=True, with_starts=False):
    """The prologue of sequence_cases.draw_ops (3 and 5 steps at op boundaries) with the refusal that needs a handle without a
    held-out set, then every planted block in a drawn order with drawn fillers between them."""
    d = _Draw2(seed, fgsm)
    d.which = 0
    d.add("train_range", first=0, B=17, n_steps=3); d.add("get_weights")
    d.add("step_host", **d.host(16)); d.add("refused2", kind="no_held_out", call="")
    d.add("step_range", first=d.first(33), n=33); d.add("get_momentum")
    blocks = _blocks2()
    fillers = [int(r) for r in d.rng.permutation(N_FILLERS)]
    d.starts = []
    # (H13 first, while the budget of a few steps is small: stale sums of a narrow sigmoid layer move a step by little)
    for i in [1] + [int(j) for j in d.rng.permutation(len(blocks)) if j != 1]:
        d.starts.append(len(d.ops))
        blocks[int(i)](d)
        if fillers and d.rng.random() < 0.4:
            d.filler2(fillers.pop())
    while fillers:
        d.filler2(fillers.pop())
    d.add("get_weights")
    return (d.ops, d.starts) if with_starts else d.ops


# ---- the hazards a sequence contains ----------------------------------------------------------------------------------------------
def _last_block(kw):
    return blocks_of(kw["first"], kw["n"])[-1]


def hazards2(ops):
    """{hazard: [op indices]} of a sequence of the second draw, from the op list alone"""
    found = {}
    def hit(h, i): found.setdefault(h, []).append(i)
    at = lambda j: ops[j] if 0 <= j < len(ops) else ("", {})
    T = lambda op: op[1]["op"] if op[0] == "teacher" else ("", {})
    prepared, src, hint, before_loop = None, None, None, None      # the batch a step prepared, by what, the pending hint
    t_prepared, t_hint, held = None, None, 0
    for i, (name, kw) in enumerate(ops):
        prev, nxt, nxt2 = at(i - 1), at(i + 1), at(i + 2)
        if name == "upload_held_out": held = kw["size"]
        # H11
        if name == "step_host" and nxt[0] in NEW_OPS and nxt[0] != "teacher":
            f = nxt[0]
            if f == "distill": f += ":" + nxt[1]["teacher"]
            if f == "refused2":
                f = nxt[1]["call"] if nxt[1]["kind"] == "fgsm" and nxt[1]["call"] else "refused2:" + nxt[1]["kind"]
            hit("H11:" + f, i)
        if T((name, kw))[0] == "step_host" and nxt[0] == "distill" and nxt[1]["teacher"] == "other":
            hit("H11:distill:teacher", i); hit("H16:pending", i)
        # H12
        if name in GRAD_ONLY and _last_block(kw)[1] in (33, 40):
            if nxt[0] == "step_range" and 3 <= nxt[1]["n"] <= 5 and nxt2[0] == "get_weights": hit("H12:step", i)
            if prev[0] == "compute_gradient_range" and nxt[0] == "apply_update": hit("H12:update", i)
        # the batch prepared ahead
        key = (kw["first"], kw["n"]) if name == "step_range" else (kw["first"], kw["B"]) if name == "train_range" else None
        if key is not None and key == before_loop and prev[0] in ("train_fgsm", "refused2"): hit("H19:chain", i)
        if key is not None and key == prepared:
            if prev[0] in GRAD_ONLY and not prev[1].get("held"):
                hit("H13:loop" if src == "train_range" else "H13:b" if _last_block(prev[1]) == key else "H13:a", i)
            if prev[0] in ("set_targets", "distill"):
                covers = prev[1]["first"] <= key[0] and key[0] + key[1] <= prev[1]["first"] + prev[1]["n"]
                hit("H15:" + prev[0] if covers else "H15:beside", i)
            if prev[0] == "upload_held_out": hit("H17:upload", i)
            if prev[0] == "evaluate_set" and prev[1]["held"] and prev[1]["n"] > MAX_BATCH: hit("H17:eval", i)
        if name == "step_range" and prev[0] == "step_range" and at(i - 2)[0] == "distill" and at(i - 2)[1]["teacher"] == "self" \
                and at(i - 3)[0] == "hint" and (at(i - 3)[1]["first"], at(i - 3)[1]["n"]) == key:
            hit("H16:self", i)
        if name == "evaluate_set" and kw["n"] > MAX_BATCH and prev[0] in ("set_targets", "distill") and at(i - 2) == (name, kw): hit("H15:eval", i)
        if name in ("fgsm_range", "evaluate_fgsm") and kw["held"]:
            if nxt[0] == "step_host" and nxt[1]["n"] == _last_block(kw)[1] and nxt2[0] == "propagate": hit("H14", i)
            if nxt[0] == "propagate": hit("H14:shadow", i)
        if name == "upload" and held == ROWS == sq.rows_of(kw["which"]) and nxt[0] == nxt2[0] == "evaluate_set" \
                and nxt[1]["held"] and not nxt2[1]["held"] and nxt[1]["n"] == nxt2[1]["n"] == ROWS:
            hit("H17:same-count", i)
        if name == "train_sampled" and prev[0] == "sample" and at(i - 2)[0] == "train_held_out" and 16 < at(i - 2)[1]["iters"] < 48: hit("H18", i)
        if name in ("train_fgsm", "refused2") and kw.get("call", "train_fgsm") == "train_fgsm" and (prev[0] == "step_range" and at(i - 2)[0] == "hint"
                                                                                  or prev[0] == "step_host" and at(i - 3)[0] == "hint"):
            hit("H19:hinted", i)
        # the teacher's chain
        tn, tkw = T((name, kw))
        if tn == "hint": t_hint = (tkw["first"], tkw["n"])
        elif tn == "step_range":
            if (tkw["first"], tkw["n"]) == t_prepared and prev[0] == "distill" and prev[1]["teacher"] == "other" and T(nxt)[0] == "loss_range":
                hit("H16", i)
            t_prepared, t_hint = t_hint, None
        elif tn in sq.TRAINING: t_prepared, t_hint = None, None
        # what this op leaves prepared
        if name == "hint": hint = (kw["first"], kw["n"])
        elif name in ("step_range", "apply_update"): prepared, src, hint, before_loop = hint, "hint", None, None
        elif name == "train_range":
            nb = ROWS // kw["B"]
            prepared, src, hint, before_loop = (((kw["first"] // kw["B"] + kw["n_steps"]) % nb) * kw["B"], kw["B"]), "train_range", None, None
        elif name == "train_fgsm" or (name == "refused2" and kw["kind"] == "fgsm" and kw["call"] == "train_fgsm"):
            before_loop, prepared, hint = before_loop or prepared, None, None
        elif name == "step_host" and nxt[0] == "refused2" and nxt[1].get("call") == "train_fgsm":
            before_loop, prepared, hint = prepared, None, None
        elif name in sq.TRAINING + NEW_TRAINING or name in ("forget", "upload"): prepared, hint, before_loop = None, None, None
        elif name in GRAD_ONLY and (kw.get("held") or _last_block(kw) != prepared):
            if not kw.get("held") and prepared is not None and nxt[0] == "step_range" and (nxt[1]["first"], nxt[1]["n"]) == prepared:
                continue                                         # (H13 a: the step that follows is still the hazard)
            prepared = None
    return found


HAZARDS_ALL = ["H11:" + f for f in H11_FOLLOWERS] + ["H12:step", "H12:update", "H13:a", "H13:b", "H13:loop", "H15:set_targets", "H15:distill",
                                                     "H15:beside", "H15:eval", "H16", "H16:pending", "H16:self", "H17:upload", "H17:eval",
                                                     "H17:same-count", "H18", "H19:hinted", "H19:chain"]
HAZARDS_FGSM = ["H14", "H14:shadow"]                           # need a perturbing call


# ---- the model ------------------------------------------------------------------------------------------------------------------
def best_point(hits, loss, rule):
    """the header's rule for the running best, in point order"""
    at = -1
    for p in range(len(loss)):
        if rule == "loss": better = not np.isnan(loss[p]) and (at < 0 or loss[p] < loss[at])
        else: better = at < 0 or hits[p] > hits[at] or (hits[p] == hits[at] and loss[p] < loss[at])
        if better: at = p
    return at


class Model2(sq.Model):
    """sequence_cases.Model with the new ops and F9 .. F17; every gradient by np_oracle (targets need not be one-hot)."""

    def __init__(self, oracle_mod, case, fault=None, reads=True, with_teacher=True):
        super().__init__(oracle_mod, case, fault, reads)
        self.Xo = self.Yo = None           # the held-out set
        self.left = None                   # dict(X, Y, key): the last block of a gradient-only call on training rows, for the step behind it
        self.staged = None                 # the perturbed rows a perturbing call left in the staging rows
        self.new_export = False            # self.exported is a new call's
        self.borrowed = None               # F14: (first, n, X, Y) of the student's rows the teacher was run on
        self.kind = 0 if self.out_kind == cc.OUT_SOFTMAX_CE else 1
        self.teacher = Model2(oracle_mod, teacher_case(case), fault, reads, with_teacher=False) if with_teacher else None
        self.group_W = [sq.start_weights(oracle_mod, self.dims, seed=s) for s in GROUP_SEEDS] if with_teacher else []

    # -- arithmetic ---------------------------------------------------------------------------------------------------------------
    def _losses(self, X, Y):
        if self.bf16:
            return super()._losses(X, Y)
        return np_oracle.loss(self._Ws(), X, Y, self.inner, self.kind, self.last)

    def _gradient(self, X, Y, W1=None, X1=None):
        """X1: the first-layer sums taken from THESE rows (the gradient product of layer 0 reads the batch's own)"""
        if X1 is None and W1 is None:
            fn = np_oracle.gradient_bf16 if self.bf16 else np_oracle.gradient
            return fn(self._Ws(), X, Y, self.inner, self.kind, self.last)
        if X1 is None:
            return super()._gradient(X, Y, W1)
        q = np_oracle.bf16_round if self.bf16 else (lambda a: a)
        Ws = self._Ws()
        Z = [np.asarray(X, dtype=np.float64)]
        for l, Wl in enumerate(Ws):
            src = np.asarray(X1, dtype=np.float64) if l == 0 else Z[-1]
            Z.append(q(np_oracle.act(self.inner, src)) @ q(Wl))
        if self.kind == 0:
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

    def input_gradient(self, X, Y, W=None):
        fn = igc.input_gradient_bf16 if self.bf16 else igc.input_gradient
        return fn(self._Ws(W), X, Y, self.inner, self.kind, self.last)

    def outputs_of(self, X, who):
        """the teacher's outputs on the student's rows"""
        if who == "self": return self._forward(X)[0]
        if who == "other": return self.teacher._forward(X)[0]
        keep, out = self.W, []
        for W in self.group_W:
            self.W = W; out.append(self._forward(X)[0])
        self.W = keep
        return np.mean(out, axis=0)

    def _train(self, i, X, Y, key=None, host=False, X1=None):
        n, W1 = len(X), None
        before = (self.W, self.V)
        if key is not None and self.ahead is not None and self.ahead["key"] == key:
            if self.ahead["replaced"]:
                self._event("F1", i)
                if self.fault == "F1": W1 = np_oracle.split(self.ahead["W"], self.dims)[0]
            if self.ahead["uploaded"]:
                self._event("F7", i)
                if self.fault == "F7": X, Y = self.ahead["X"], self.ahead["Y"]
            if self.ahead.get("retargeted"):
                self._event("F13", i)
                if self.fault == "F13": Y = self.ahead["Y"]
        if key is not None and self.left is not None and self.left["key"] != key and len(self.left["X"]) == n:
            self._event("F11", i)
            if self.fault == "F11": X1 = self.left["X"]
        if host and self.staged is not None and len(self.staged) == n:
            self._event("F12", i)
            if self.fault == "F12": X1 = self.staged
        if self.borrowed is not None and key is not None:
            self._event("F14", i)
            if self.fault == "F14": X, Y = self.borrowed[2][key[0]:key[0] + n], self.borrowed[3][key[0]:key[0] + n]
        add = None
        if self.exported is not None:
            self._event("F10" if self.new_export else "F4", i)
            if self.fault == ("F10" if self.new_export else "F4"): add = self.exported
        self.exported, self.left, self.staged = None, None, None
        G = self._gradient(X, Y, W1, X1)
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

    def _evaluate(self, X, Y, kind):
        lab, safe = self._labels(X)
        out = dict(labels=lab, safe=safe, expected=stc.expected_class(Y))
        if kind == "evaluate":
            out.update(hits=int((lab == out["expected"]).sum()), unsafe=int((~safe).sum()), loss_sum=float(self._losses(X, Y).sum()))
        return out

    def _retarget(self, first, n, Ynew):
        Y = np.array(self.Y)
        Y[first:first + n] = Ynew
        Y.setflags(write=False)
        self.Y = Y
        if self.ahead is not None:
            f, m = self.ahead["key"]
            if first < f + m and f < first + n: self.ahead["retargeted"] = True

    def set_device_targets(self, first, Y):
        """the GPU test hands over the rows the device holds after a distillation"""
        self._retarget(first, len(Y), Y)

    def _rows_of_set(self, held):
        return (self.Xo, self.Yo) if held else (self.X, self.Y)

    def _gradient_only(self, i, kw, name):
        """input_gradient_range / fgsm_range / evaluate_fgsm: per block the gradient (and the perturbation) at the weights as they are"""
        held = bool(kw.get("held"))
        Xs, Ys = self._rows_of_set(held)
        out, parts, adv = {}, [], None
        for f, m in blocks_of(kw["first"], kw["n"]):
            X, Y = Xs[f:f + m], Ys[f:f + m]
            if self.reads:
                g = self.input_gradient(X, Y) if name != "evaluate_fgsm" else None
                adv = clip_rows(X, g if kw.get("signed") else None) if name != "input_gradient_range" else None
                parts.append((X, Y, g, adv))
        f, m = blocks_of(kw["first"], kw["n"])[-1]
        X, Y = Xs[f:f + m], Ys[f:f + m]
        self.G = self.exported = self._gradient(X, Y)
        self.new_export, self.prev = True, (X, Y)
        if name != "input_gradient_range":
            self.staged = clip_rows(X, self.input_gradient(X, Y) if kw.get("signed") else None)
        if held:
            self.ahead = None
        else:
            self.left = dict(X=X, Y=Y, key=(f, m))
            self.ahead = None if self.ahead is None or self.ahead["key"] != (f, m) else self.ahead
        if self.reads:
            if name == "input_gradient_range":
                out["grad_in"] = np.concatenate([p[2] for p in parts])
            elif name == "fgsm_range":
                out["rows"] = np.concatenate([p[3] for p in parts])
                if kw.get("signed"):
                    g, a0 = np.concatenate([p[2] for p in parts]), np.concatenate([p[0] for p in parts])
                    out["decided"], out["grad_in"] = ac.decided(g, a0, self.inner, self.bf16), g
            else:
                ev = [self._evaluate(p[3], p[1], "evaluate") for p in parts]
                out.update(hits=sum(e["hits"] for e in ev), unsafe=sum(e["unsafe"] for e in ev), loss_sum=sum(e["loss_sum"] for e in ev),
                           safe=np.concatenate([e["safe"] for e in ev]))
        return out

    # -- one op -------------------------------------------------------------------------------------------------------------------
    def apply(self, i, op):
        name, kw = op
        if name == "teacher":
            tn, tkw = kw["op"]
            r = self.teacher.apply(i, (tn, tkw))
            if tn == "loss_range" and self.teacher.borrowed is not None:
                self.teacher._event("F14", i)
                if self.fault == "F14":
                    b = self.teacher.borrowed
                    r["loss"] = self.teacher._losses(b[2][tkw["first"]:tkw["first"] + tkw["n"]], b[3][tkw["first"]:tkw["first"] + tkw["n"]])
                self.teacher.borrowed = None
            return dict({"T" + k: v for k, v in r.items()}, time=self.time, steps=self.steps, Tsteps=self.teacher.steps)
        if name in sq.EVALS:                                   # (the expected class of a rewritten row: the header's rule)
            return self.apply(i, ("evaluate_set", dict(kw, kind="evaluate" if name in ("count_hits", "evaluate") else name, held=False)))
        if name not in NEW_OPS:
            if name not in sq.TRAINING + ("get_weights", "get_momentum", "hint", "synchronize", "advance_time", "timing", "specialize", "save", "sample"):
                self.left = self.staged = None
            if name in ("weight_gradient", "compute_gradient_range"): self.new_export = False
            return super().apply(i, op)
        out = {}
        if "first" in kw and name != "refused2":               # (the draw keeps every range inside its set)
            assert 0 <= kw["first"] and kw["first"] + kw["n"] <= len(self._rows_of_set(kw.get("held"))[0]), (i, op)
        pend, self.pending = self.pending, None
        early = pend is not None and name in F9_READS
        if early:
            self._event("F9", i)
            if self.fault == "F9": now, (self.W, self.V) = (self.W, self.V), (pend["W"], pend["V"])
        if name not in ("fgsm_range", "evaluate_fgsm", "train_fgsm"):
            self.staged = None
        if name == "input_gradient":
            X, Y = self.Xh[kw["off"]:kw["off"] + kw["n"]], self.Yh[kw["off"]:kw["off"] + kw["n"]]
            self.G = self.exported = self._gradient(X, Y)
            self.new_export, self.prev, self.ahead, self.left = True, (X, Y), None, None
            if self.reads: out["grad_in"] = self.input_gradient(X, Y)
        elif name in GRAD_ONLY:
            out = self._gradient_only(i, kw, name)
        elif name == "get_targets":
            Ys = self._rows_of_set(kw["held"])[1]
            out["targets"] = np.array(Ys[kw["first"]:kw["first"] + kw["n"]])
        elif name == "propagate_set":
            if self.reads: out["out"] = self._forward(self._rows_of_set(kw["held"])[0][kw["first"]:kw["first"] + kw["n"]])[0]
        elif name == "evaluate_set":
            Xs, Ys = self._rows_of_set(kw["held"])
            if kw["held"] and len(Xs) == len(self.X):
                self._event("F15", i)
                if self.fault == "F15": Xs, Ys = self.X, self.Y
            if self.reads: out = self._evaluate(Xs[kw["first"]:kw["first"] + kw["n"]], Ys[kw["first"]:kw["first"] + kw["n"]], kw["kind"])
        elif name == "upload_held_out":
            self.Xo, self.Yo = held_set(self.case["seed"], kw["size"], self.dims[0], self.dims[-1])
        elif name == "set_targets":
            self._retarget(kw["first"], kw["n"], target_rows(self.case["seed"], kw["tseed"], kw["n"], self.dims[-1]))
        elif name == "distill":
            f, n, keep = kw["first"], kw["n"], kw["keep"]
            t_model = self.teacher if kw["teacher"] == "other" else None
            if t_model is not None:
                t_model.pending = None                         # (its deferred update is applied first: the model's is applied at once)
                t_model.borrowed = (f, n, self.X, self.Y)
            if keep != 1.0:
                self._retarget(f, n, keep * self.Y[f:f + n] + (1.0 - keep) * self.outputs_of(self.X[f:f + n], kw["teacher"]))
            out["targets"] = np.array(self.Y[f:f + n])
        elif name == "train_held_out":
            hits, unsafe, loss, Ws = [], [], [], []
            iters, every = kw["iters"], kw["every"]
            Vs = []
            for it in range(1, iters + 1):
                idx = (self.each if kw.get("each") else self.sampler).sample(kw["B"])
                self._train(i, self.X[idx], self.Y[idx])
                Vs.append(self.V)
                Ws.append(self.W)
                if (it % every == 0 or it == iters) and self.reads:
                    ev = self._evaluate(self.Xo[:kw["held_rows"]], self.Yo[:kw["held_rows"]], "evaluate")
                    hits.append(ev["hits"]); unsafe.append(ev["unsafe"]); loss.append(ev["loss_sum"])
            self._event("F17", i)
            if self.fault == "F17" and iters > 1: self.V = Vs[-2]
            if self.reads:
                points = [min((p + 1) * every, iters) for p in range(len(hits))]
                best = best_point(hits, loss, kw["rule"])
                out.update(curve_hits=np.array(hits), curve_unsafe=np.array(unsafe), curve_loss=np.array(loss), best=best, held_rows=kw["held_rows"])
                self._event("F16", i)
                at = points[best] - 1
                if self.fault == "F16": at = at + 1 if at + 1 < iters else at - 1
                out["best_W"] = Ws[at]
                # the decision is the model's to check where no other point comes within the budgets of the best
                l = np.array(loss)
                tol = sq.LOSS_RTOL * np.abs(l) + sq.LOSS_ATOL * kw["held_rows"]
                others = [p for p in range(len(l)) if p != best]
                out["best_clear"] = (kw["rule"] == "loss" and all(l[p] - tol[p] > l[best] + tol[best] for p in others)) or \
                                    (kw["rule"] == "hits" and max(unsafe) == 0 and all(hits[p] != hits[best] for p in others))
        elif name == "train_fgsm":
            Vs = []
            for _ in range(kw["iters"]):
                idx = self.sampler.sample(kw["B"])
                X = self.X[idx]
                self._event("F12", i)
                self._train(i, clip_rows(X), self.Y[idx], X1=X if self.fault == "F12" else None)
                Vs.append(self.V)
            self._event("F17", i)
            if self.fault == "F17" and kw["iters"] > 1: self.V = Vs[-2]
        if early and self.fault == "F9":
            self.W, self.V = now
        out["time"], out["steps"] = self.time, self.steps
        return out


is_checkpoint = sq.is_checkpoint


# ---- the budgets: one function for the GPU test and for the fault factors ---------------------------------------------------------
def fractions(case, got, want, steps):
    """[(what, err / budget)] for everything op results `got` and `want` share that has a budget (f32 against fp64).  Weight-like
    entries (W, V, best_W, TW, TV) take W_ATOL x steps so far; the others the suite's budget for their kind."""
    out = []
    w_budget = sq.W_ATOL * max(steps, 1)
    for k, what in (("W", "weights"), ("V", "momentum"), ("best_W", "best weights")):
        if k in got and k in want and got[k] is not None: out.append((what, np.abs(got[k] - want[k]).max() / w_budget))
    for k, what in (("TW", "teacher weights"), ("TV", "teacher momentum")):
        if k in got and k in want: out.append((what, np.abs(got[k] - want[k]).max() / (sq.W_ATOL * max(want.get("Tsteps", 1), 1))))
    if "out" in got: out.append(("outputs", np.abs(got["out"] - want["out"]).max() / sq.OUT_ATOL))
    for k in ("loss", "Tloss"):
        if k in got: out.append(("losses", (np.abs(got[k] - want[k]) / (sq.LOSS_RTOL * np.abs(want[k]) + sq.LOSS_ATOL)).max()))
    if "loss_sum" in got:
        n = want["safe"].size
        out.append(("validation", abs(got["loss_sum"] - want["loss_sum"]) / n / (sq.LOSS_RTOL * abs(want["loss_sum"]) / n + sq.LOSS_ATOL)))
    if "hits" in got:                                          # |difference| <= the count of unsafe rows, as a fraction of integers
        out.append(("hits", abs(int(got["hits"]) - want["hits"]) / (want["unsafe"] + 0.5)))
    if "curve_loss" in got:
        n = want["held_rows"]
        out.append(("held-out curve", (np.abs(got["curve_loss"] - want["curve_loss"]) / n
                                       / (sq.LOSS_RTOL * np.abs(want["curve_loss"]) / n + sq.LOSS_ATOL)).max()))
    if "grad_in" in got and "grad_in" in want and "rows" not in got:
        err, bud = igc.within(got["grad_in"], want["grad_in"], case["dtype"] == "bf16")
        out.append(("input gradient", err / bud))
    return out


# ---- proof that the budgets see the faults ------------------------------------------------------------------------------------------
_STATE2 = sq._STATE + ("Xo", "Yo", "left", "staged", "new_export", "borrowed")
OWN_RESULT = ("F9", "F15", "F16")          # looked for in the result of the op itself


def _snapshot(m):
    s = {k: getattr(m, k) for k in _STATE2}
    s["saves"] = dict(m.saves)
    s["ahead"] = None if m.ahead is None else dict(m.ahead)
    s["teacher"] = None if m.teacher is None else _snapshot(m.teacher)
    return s


def _restore(m, s):
    for k in _STATE2:
        setattr(m, k, s[k])
    m.saves = dict(s["saves"]); m.ahead = None if s["ahead"] is None else dict(s["ahead"])
    if m.teacher is not None: _restore(m.teacher, s["teacher"])


def _draws(op):
    name, kw = op
    return {"sample": 1, "train_sampled": kw.get("iters"), "train_observed": kw.get("iters"), "train_held_out": kw.get("iters"),
            "train_fgsm": kw.get("iters")}.get(name, 0)


def _sampler_at(oracle_mod, case, i0):
    s = oracle_mod.Sampler(ROWS, seed=sq.SAMPLER_SEED)
    for op in case["ops"][:i0]:
        for _ in range(_draws(op)):
            s.sample(op[1]["B"])
    return s


def run_model(oracle_mod, case):
    """The correct model over the sequence: per-op results (W, V at checkpoints; the teacher's at its own ops) and, for every fault,
    the (op index, state in front of it) of every occurrence of its hazard."""
    ops = case["ops"]
    m = Model2(oracle_mod, case)
    results, snaps = [], {}
    for i, op in enumerate(ops):
        snap = _snapshot(m)
        n_ev, t_ev = len(m.events), len(m.teacher.events)
        r = m.apply(i, op)
        for name in {e[0] for e in m.events[n_ev:] + m.teacher.events[t_ev:]}:
            snaps.setdefault(name, []).append((i, snap))
        if is_checkpoint(i, ops) or op[0] in ("get_weights", "get_momentum"):
            r["W"], r["V"] = m.W.copy(), m.V.copy()
        if op[0] == "teacher" and op[1]["op"][0] == "get_weights":
            r["TV"] = m.teacher.V.copy()
        results.append(r)
    return results, snaps


def _faulty_from(oracle_mod, case, fault, i0, snap):
    m = Model2(oracle_mod, case, fault=fault)
    _restore(m, snap)
    m.sampler = _sampler_at(oracle_mod, case, i0)
    return m


def fault_factor(oracle_mod, case, fault, results, snaps, every=False):
    """How far, in budgets, the model with `fault` lies from the correct one at the first check behind the fault's hazard: for
    OWN_RESULT faults the hazard op's own result at the first occurrence (every=True: the least over every occurrence); for the others
    the first checkpoint, get_weights or get_momentum (F14: the teacher's first loss_range or get_weights) at or behind the first
    occurrence.  None: the sequence has no such hazard."""
    if fault not in snaps:
        return None
    ops = case["ops"]
    if fault in OWN_RESULT:
        least = np.inf
        # (an evaluation that returns labels alone is exact on safe rows: no budget to measure in)
        measurable = [(i0, s) for i0, s in snaps[fault] if not (ops[i0][0] == "evaluate_set" and ops[i0][1]["kind"] != "evaluate")]
        for i0, snap in measurable[:None if every else 1]:
            m = _faulty_from(oracle_mod, case, fault, i0, snap)
            r = m.apply(i0, ops[i0])
            if fault == "F16": r = {"best_W": r["best_W"]}
            fr = fractions(case, r, results[i0], results[i0]["steps"])
            least = min(least, max(f for _, f in fr))
        return float(least)
    i0, snap = snaps[fault][0]
    m = _faulty_from(oracle_mod, case, fault, i0, snap)
    for i in range(i0, len(ops)):
        r = m.apply(i, ops[i])
        if fault == "F14":                                       # the teacher's loss_range or get_weights, whichever comes first
            if ops[i][0] == "teacher" and ops[i][1]["op"][0] in ("loss_range", "get_weights"):
                r = dict(r, TV=m.teacher.V)
                return float(max(f for _, f in fractions(case, r, results[i], results[i]["steps"])))
            continue
        keys = {"get_weights": ("W",), "get_momentum": ("V",)}.get(ops[i][0], ("W", "V") if is_checkpoint(i, ops) else ())
        if keys:
            got = dict(W=m.W, V=m.V)
            return float(max(f for _, f in fractions(case, {k: got[k] for k in keys}, results[i], results[i]["steps"])))
    return 0.0


# ---- groups ---------------------------------------------------------------------------------------------------------------------
GROUPS = sq.GROUPS                 # one sequence per group shape
N_GROUP = len(GROUPS)
GROUP_OPS2 = ("g_train_range", "g_train_sampled", "g_set_targets", "g_upload_held_out", "g_evaluate_set", "g_confusion_set", "g_ensemble_set",
              "g_train_held_out", "g_input_gradient", "member")
PAIRS2 = ("targets-between-loops", "held-out-upload-between-loops", "held-out-evaluation-between-loops", "member-gradient-between-loops",
          "keep-best-then-shared", "keep-best-then-each", "keep-best-then-sizes")
MEMBER_READS = ("input_gradient_range", "get_targets", "propagate_set", "evaluate_set")


def group_case(i):
    name, dims, inner, out_kind, last, dtype, K = GROUPS[i]
    seed = 9800 + i
    return dict(id="%s-new" % name, net=name, dims=list(dims), inner=inner, out_kind=out_kind, last=last, dtype=dtype,
                seed=seed, K=K, wseeds=[k + 1 for k in range(K)], each_seeds=[11 + k for k in range(K)],
                steps=[cc.STEP * (1.0 - 0.03 * k) for k in range(K)], momenta=[cc.MOMENTUM - 0.01 * k for k in range(K)],
                ops=draw_group_ops(seed, K))


def member_case(case, k):
    return dict(case, id="%s[%d]" % (case["id"], k), wseed=case["wseeds"][k], each_seed=case["each_seeds"][k], step=case["steps"][k],
                momentum=case["momenta"][k], ops=[member_op(op, k) for op in case["ops"]])


def member_op(op, k):
    """the call a lone net makes in member k's place (None: none)"""
    name, kw = op
    if name == "member": return kw["op"] if kw["k"] == k else None
    if name == "g_set_targets": return ("set_targets", kw)
    if name == "g_upload_held_out": return ("upload_held_out", kw)
    if name == "g_evaluate_set": return ("evaluate_set", dict(kw, kind="evaluate"))
    if name == "g_confusion_set": return ("evaluate_set", dict(kw, kind="confusion"))
    if name == "g_input_gradient": return ("input_gradient_range", kw)
    if name == "g_train_held_out": return ("train_held_out", dict(kw, B=kw["B"][k] if isinstance(kw["B"], list) else kw["B"], each=True))
    if name == "g_ensemble_set": return None
    return sq.member_op(op, k)


def draw_group_ops(seed, K):
    """About 40 calls on a group: each new group call and a member's input_gradient_range between two grouped training calls on the
    batch the first prepared, the keep-best loop in front of g_train_sampled in each mode, and the new reads alone."""
    d = _Draw2(seed, False)
    mid, last = K // 2, K - 1
    member = lambda k, name, **kw: d.add("member", k=k, op=(name, kw))
    d.add("g_train_range", first=0, B=17, n_steps=3)
    d.held = 57; d.add("g_upload_held_out", size=57)

    def between(what):
        call, nxt = d.range_call(2)
        d.add("g_train_range", **call)
        if what == "targets":
            d.tseed += 1; f = max(nxt[0] - 2, 0)
            d.add("g_set_targets", first=f, n=nxt[0] + nxt[1] - f, tseed=d.tseed)
        elif what == "upload":
            d.held = d.pick((57, 101)); d.add("g_upload_held_out", size=d.held)
        elif what == "eval":
            n = int(d.rng.integers(MAX_BATCH + 1, d.held + 1))
            d.add("g_evaluate_set", held=True, first=int(d.rng.integers(0, d.held - n + 1)), n=n)
        else:
            f, n = d.ending_at(int(d.rng.integers(0, ROWS - 33)), 33)
            member(d.pick((0, mid, last)), "input_gradient_range", first=f, n=n)
        d.add("g_train_range", first=nxt[0], B=nxt[1], n_steps=int(d.rng.integers(1, 4)))

    def keep_best(mode, long):
        sizes = [d.pick((5, 16, 17, 33)) for _ in range(K)]
        d.add("g_train_held_out", iters=int(d.rng.integers(17, 21)) if long else int(d.rng.integers(3, 6)), B=sizes if mode == "sizes" else d.pick((15, 17)),
              every=d.pick((1, 3, 7)), held_rows=d.pick((7, d.held)), rule=d.pick(("loss", "hits")))
        d.add("g_train_sampled", mode=mode, iters=int(d.rng.integers(2, 5)), B=[d.pick(BATCHES) for _ in range(K)] if mode == "sizes" else d.pick((16, 33)))

    def reads():
        n = d.pick((5, 17, 40))
        d.add("g_confusion_set", held=True, first=int(d.rng.integers(0, d.held - n + 1)), n=n)
        d.add("g_ensemble_set", held=True, first=0, n=d.held)
        d.add("g_input_gradient", first=d.first(n + MAX_BATCH), n=n + MAX_BATCH)
        member(last, "propagate_set", first=0, n=d.held, held=True); member(0, "get_targets", first=d.first(n), n=n, held=False)
        member(mid, "evaluate_set", kind="evaluate", held=True, first=0, n=d.held)
        d.add("g_evaluate_set", held=False, first=0, n=ROWS)

    long = int(d.rng.integers(0, 3))
    blocks = [lambda w=w: between(w) for w in ("targets", "upload", "eval", "member")] + \
             [lambda j=j, m=m: keep_best(m, j == long) for j, m in enumerate(("shared", "each", "sizes"))] + [reads]
    for i in d.rng.permutation(len(blocks)):
        blocks[int(i)]()
    return d.ops


def group_pairs(ops):
    """{pair: [op indices]} of the planted PAIRS2 in a group sequence"""
    found, ahead = {}, None
    def hit(h, i): found.setdefault(h, []).append(i)
    for i, (name, kw) in enumerate(ops):
        prev = ops[i - 1] if i else ("", {})
        if name == "g_train_range":
            if ahead == (kw["first"], kw["B"]):
                if prev[0] == "g_set_targets" and prev[1]["first"] <= kw["first"] and kw["first"] + kw["B"] <= prev[1]["first"] + prev[1]["n"]:
                    hit("targets-between-loops", i)
                if prev[0] == "g_upload_held_out": hit("held-out-upload-between-loops", i)
                if prev[0] == "g_evaluate_set" and prev[1]["held"] and prev[1]["n"] > MAX_BATCH: hit("held-out-evaluation-between-loops", i)
                if prev[0] == "member" and prev[1]["op"][0] == "input_gradient_range": hit("member-gradient-between-loops", i)
            nb = ROWS // kw["B"]
            ahead = (((kw["first"] // kw["B"] + kw["n_steps"]) % nb) * kw["B"], kw["B"])
        elif name == "g_train_sampled":
            if prev[0] == "g_train_held_out": hit("keep-best-then-" + kw["mode"], i)
            ahead = None
        elif name == "g_train_held_out":
            ahead = None
    return found
