"""Fixtures of the soft-target tests (tests/test_soft_targets_cpu.py pins them and shows that the fault models below leave the
budgets on them; tests/test_soft_targets_gpu.py runs them through every head that reads expected rows on the device): small
nets with ordinary weights whose expected rows Y are NOT one-hot.  The reference sets no condition on Y -- calculateLoss is
-sum_j y_j ln p_j (SCE:213-217) or sum_j (a_j - y_j)^2 / 2 (GNN:236-239), the output delta p - y (SCE:249-251) or
(a - y) f'(z) (GNN:267-271) -- and the rest of the suite builds Y as np.eye(d)[labels], on which a loss formed as
lse - sum y z, a skip of terms by `y > 0` or `y == 1`, a head that takes the label column, a clamp of y to [0, 1], targets
narrowed to bf16 and a per-row quantity taken from a neighbouring row all give the right numbers.  No GPU code: numpy and
tests/np_oracle.py.

NETS.  The geometry of tests/saturation_cases.py with ordinary weights: the f32 Random(seed) draw, each layer scaled to
GAIN[name] / sqrt(fan-in) (saturation_cases._scaled_draw), logits of order one to three.  Inputs: U[0, 1) with half the entries
exactly zero, f32-rounded.

TARGETS of the softmax fixtures.  Row r is of kind r % 6 -- every 4-row block holds four kinds, every 16-row group all six:
  0 SMOOTHED  0.9 on a drawn class, 0.1 / (d - 1) elsewhere
  1 TEACHER   the softmax of 2 N(0, 1) logits: dense, sum 1
  2 TWO_ONES  two exact 1.0s: sum 2.  Every other such row has its LAST one on the fp64 oracle's label (the expected class by
              MT:186-188 is the last exact 1.0: a hit on a row that is not one-hot), the others on two drawn classes
  3 ZERO      all zero
  4 FREE      U(-0.5, 1.5) per entry: negatives, values above 1, a sum that is not 1
  5 ONE_HOT
General fixtures: FREE on even rows, ONE_HOT on odd rows.  Every target is rounded to f32 before anything sees it.

BUDGETS.  saturation_cases.BUDGET, and for General nets the General numbers of tests/test_saturation_gpu.py::_out_bounds.  The
relative loss term is taken on sum_j |y_j (lse - z_j)|, the terms before they cancel: |loss| on rows without negative entries,
what an f32 sum of signed terms can hold on a FREE row.  No other number.

Measured on the CPU (tests/test_soft_targets_cpu.py prints them), as fractions of the budgets:
  float32 restatement of the reference's formulas .......... <= 0.028 (W after the steps: the f32 masters' own rounding; else <= 0.023)
  bf16 oracle under jitter 1e-6, four seeds ................ <= 0.21 (gradients of G4s; outputs, loss, W, V <= 0.11)
  fault models, smallest distance over the fixtures, loss / gradient, in budgets of the dtype:
    f32   sum1 7 200  y>0 335  y==1 4 100  onehot 4 800 / 17 000  clip 35 / 1 700  ybf16 6 / 8  rowmix 9 400 / 7 100
    bf16  sum1 1 400  y>0 6.9  y==1 96     onehot 48 / 131        clip 0.7 / 13    ybf16 0.13 / 0.23 (not visible)  rowmix 94 / 53
  (clip in bf16 leaves the loss budget by 4 or more on every fixture but T1100, whose FREE row has 1100 terms that nearly cancel
  under the clamp; its gradient leaves by 57 budgets there.)
"""
import numpy as np

from tests import np_oracle
from tests import saturation_cases as sc

LEAKY, SIGMOID, TANH, RELU, IDENT = range(5)
SCE, GENERAL = 0, 1
F32, BF16 = 0, 1
SMOOTHED, TEACHER, TWO_ONES, ZERO, FREE, ONE_HOT = range(6)
N_KINDS = 6
STEP, MOMENTUM, N_STEPS = sc.STEP, sc.MOMENTUM, sc.N_STEPS
JITTER, JITTER_SEEDS = sc.JITTER, sc.JITTER_SEEDS
BUDGET = sc.BUDGET
GENERAL_F32 = dict(p=2e-5, l_rel=1e-4, l_abs=1e-5)   # tests/test_saturation_gpu.py::_out_bounds
f32 = sc.f32

#         name     dims                      out      inner    last     rows
_TABLE = [
    ("T3",    [20, 12, 10],             SCE,     LEAKY,   IDENT,   37),
    ("T4",    [20, 12, 8, 10],          SCE,     TANH,    IDENT,   37),
    ("T16",   [20, 12, 8, 16],          SCE,     RELU,    IDENT,   37),   # 16 outputs: no padding column
    ("T132",  [20, 132, 10],            SCE,     LEAKY,   IDENT,   21),   # last hidden layer > 128: middle4's register head
    ("T17",   [20, 12, 17],             SCE,     SIGMOID, IDENT,   37),   # more than 16 outputs: middle4's general head
    ("T40",   [20, 12, 9, 8, 7, 40],    SCE,     IDENT,   IDENT,   21),
    ("T1100", [40, 24, 1100],           SCE,     LEAKY,   IDENT,   6),    # the output kernel's three-pass form
    ("TB",    [784, 100, 50, 10],       SCE,     LEAKY,   IDENT,   37),   # a prebuilt instance
    ("G4s",   [20, 12, 8, 10],          GENERAL, TANH,    SIGMOID, 37),
    ("G4t",   [20, 12, 8, 10],          GENERAL, TANH,    TANH,    37),
    ("G4i",   [20, 12, 8, 10],          GENERAL, TANH,    IDENT,   37),
    ("G17",   [20, 12, 17],             GENERAL, TANH,    IDENT,   21),   # more than 16 outputs
    ("GB",    [784, 100, 50, 10],       GENERAL, LEAKY,   SIGMOID, 37),   # a prebuilt General instance
]
NAMES = [r[0] for r in _TABLE]
SOFTMAX = [r[0] for r in _TABLE if r[2] == SCE]
GENERAL_NAMES = [r[0] for r in _TABLE if r[2] == GENERAL]
# One set of weights per fixture serves f32 and bf16.  The wide nets are drawn lower: a bf16 net's error against the fp64
# oracle follows the largest logit (tests/group_eval_cases.py), and their sums run over 784 inputs.
GAIN = {"TB": 1.0, "GB": 1.0, "T40": 1.2}
DEFAULT_GAIN = 2.0
MIN_GAP = 0.03     # of the fp64 top-2 gap: three times the bf16 margin rule at logits of 4
HELD_ROWS = 24     # the held-out rows of train_sampled_held_out: four of every kind


def kinds(rows, out_kind=SCE):
    r = np.arange(rows)
    return r % N_KINDS if out_kind == SCE else np.where(r % 2 == 0, FREE, ONE_HOT)


def expected_class(Y):
    """MT:186-188 (confusion_kernel.h: expected_class): the last index whose expected value is exactly 1, else class 0."""
    return np.array([int(np.flatnonzero(r == 1.0)[-1]) if (r == 1.0).any() else 0 for r in np.asarray(Y)])


def _inputs(seed, rows, d0):
    rng = np.random.default_rng(seed)
    return f32(rng.random((rows, d0)) * (rng.random((rows, d0)) < 0.5)), rng


def _targets(rng, kind, d, label):
    Y = np.zeros((len(kind), d))
    twos = 0
    for r, k in enumerate(kind):
        if k == SMOOTHED:
            Y[r] = 0.1 / (d - 1)
            Y[r, rng.integers(0, d)] = 0.9
        elif k == TEACHER:
            t = 2.0 * rng.standard_normal(d)
            e = np.exp(t - t.max())
            Y[r] = e / e.sum()
        elif k == TWO_ONES:
            if twos % 2 == 0 and label[r] > 0:
                Y[r, [label[r], rng.integers(0, label[r])]] = 1.0
            else:
                Y[r, rng.choice(d, 2, replace=False)] = 1.0
            twos += 1
        elif k == FREE:
            while not (Y[r].min() < 0.0 and Y[r].max() > 1.0):     # (a row of ten may lack one of the two: drawn again)
                Y[r] = rng.uniform(-0.5, 1.5, d)
        elif k == ONE_HOT:
            Y[r, rng.integers(0, d)] = 1.0
    return f32(Y)


def _label(key):
    return np.array([int(np.flatnonzero(r >= r.max())[-1]) for r in key])      # the reference's `>=` argmax


class Fixture:
    """One net, its weights (f32-exact, flat `w` and per layer `Ws`), rows X (f32-exact), expected rows Y (f32-exact), the
    target kind of every row, and the held-out rows Xh, Yh (their own draw, the same kinds)."""

    def __init__(self, oracle_mod, name, dims, out_kind, inner, last, rows, seed=1, like=None):
        """seed: the Random(seed) draw.  like: another member of a net group -- its rows and expected rows."""
        self.name, self.dims, self.out_kind, self.inner, self.last, self.rows = name, dims, out_kind, inner, last, rows
        self.Ws = [f32(W) for W in sc._scaled_draw(oracle_mod, dims, out_kind, inner, last, seed, GAIN.get(name, DEFAULT_GAIN))]
        self.w = np.concatenate([W.ravel() for W in self.Ws])
        if like is not None:
            self.X, self.Y, self.kind, self.Xh, self.Yh = like.X, like.Y, like.kind, like.Xh, like.Yh
            return
        d_out = dims[-1]
        self.kind = kinds(rows, out_kind)
        self.X, rng = self._rows(7000 + 10 * len(dims) + d_out + dims[0], rows)
        self.Y = _targets(rng, self.kind, d_out, self._labels(self.X)[0])
        self.Xh, rng = self._rows(8000 + 10 * len(dims) + d_out + dims[0], HELD_ROWS)
        self.Yh = _targets(rng, kinds(HELD_ROWS, out_kind), d_out, self._labels(self.Xh)[0])
        for a in (self.X, self.Y, self.Xh, self.Yh, self.w):
            a.setflags(write=False)

    def _labels(self, X):
        Z, out = np_oracle.forward(self.Ws, X, self.inner, self.out_kind, self.last)
        key = Z[-1] if self.out_kind == SCE else out
        return _label(key), sc._top2_gap(key)

    def _rows(self, seed, rows):
        """The first `rows` of a seeded draw of candidates whose fp64 top-2 gap exceeds MIN_GAP, so that labels can be compared
        on nearly every row (the targets are drawn afterwards and do not enter)."""
        X, rng = _inputs(seed, 8 * rows, self.dims[0])
        keep = np.flatnonzero(self._labels(X)[1] > MIN_GAP)[:rows]
        assert keep.size == rows, "fixture %s: too few candidate rows" % self.name
        return X[keep], rng

    def __repr__(self):
        return self.name

    def truth(self, dtype):
        """The oracle's verdict: computed on demand, cached, read-only."""
        key = "_truth%d" % dtype
        if not hasattr(self, key):
            setattr(self, key, Truth(self, dtype))
        return getattr(self, key)


_fixtures = {}


def fixture(oracle_mod, name, seed=1):
    """The fixture (seed 1), or the net of Random(seed) on the same rows: a further member of a net group."""
    if (name, seed) not in _fixtures:
        row = next(r for r in _TABLE if r[0] == name)
        _fixtures[(name, seed)] = Fixture(oracle_mod, *row) if seed == 1 else Fixture(oracle_mod, *row, seed=seed, like=fixture(oracle_mod, name))
    return _fixtures[(name, seed)]


def forward(fx, dtype, Ws, X, jitter=None):
    """(logits, outputs) of rows X with weights Ws: np_oracle.forward in fp64, or its bf16 form."""
    if dtype == BF16:
        Z, _, out = np_oracle.forward_bf16(Ws, X, fx.inner, fx.out_kind, fx.last, jitter=jitter)
    else:
        Z, out = np_oracle.forward(Ws, X, fx.inner, fx.out_kind, fx.last)
    return Z[-1], out


def loss_rows(fx, Z, out, Y):
    """(calculateLoss per row, sum_j |term_j| per row): SCE:213-217 as sum_j y_j (lse - z_j), GNN:236-239."""
    if fx.out_kind == SCE:
        zz = Z - Z.max(axis=1, keepdims=True)
        lse = np.log(np.exp(zz).sum(axis=1, keepdims=True))
        terms = Y * (lse - zz)
    else:
        terms = 0.5 * (out - Y) ** 2
    return terms.sum(axis=1), np.abs(terms).sum(axis=1)


def gradient(fx, dtype, Ws, X, Y, jitter=None):
    if dtype == BF16:
        return np_oracle.gradient_bf16(Ws, X, Y, fx.inner, fx.out_kind, fx.last, jitter=jitter)
    return np_oracle.gradient(Ws, X, Y, fx.inner, fx.out_kind, fx.last)


def oracle_step(fx, dtype, w, v, X, Y, step=STEP, momentum=MOMENTUM, jitter=None):
    """One gradientStep on rows X, Y."""
    if dtype == BF16:
        return np_oracle.gradient_step_bf16(w, v, fx.dims, X, Y, step, momentum, fx.inner, fx.out_kind, fx.last, jitter=jitter)
    return np_oracle.gradient_step(w, v, fx.dims, X, Y, step, momentum, fx.inner, fx.out_kind, fx.last)


def loss_at(fx, dtype, w, X, Y):
    """calculateLoss per row of X, Y with the flat weights w, and the terms' absolute sum."""
    Z, out = forward(fx, dtype, np_oracle.split(np.asarray(w, dtype=np.float64), fx.dims), X)
    return loss_rows(fx, Z, out, Y)


class Verdict:
    """The oracle on rows X, Y with the layer matrices Ws of the fixture's net (its activations and output rule are all that
    is read of `fx`).  Z: logits; out: probabilities / outputs; loss, terms: per row (loss_rows); expected (MT:186-188), label
    (the `>=` argmax) and safe rows (the project's margin rule on the top-2 gap: f32 1e-3 on the logits, 1e-4 max(1, max|a|) on
    a General net's outputs; bf16 2e-3 max|.| + 1e-3)."""

    def __init__(self, fx, dtype, Ws, X, Y, jitter=None):
        self.Z, self.out = forward(fx, dtype, Ws, X, jitter)
        self.loss, self.terms = loss_rows(fx, self.Z, self.out, Y)
        key = self.Z if fx.out_kind == SCE else self.out
        self.label = _label(key)
        self.expected = expected_class(Y)
        margin = sc._top2_gap(key)
        if dtype == BF16:
            self.safe = margin > 2e-3 * np.abs(key).max() + 1e-3
        else:
            self.safe = margin > (1e-3 if fx.out_kind == SCE else 1e-4 * max(1.0, np.abs(key).max()))

    def hits_bounds(self, rows=slice(None)):
        """[hits on safe rows, the same + unsafe rows]: what a count of label == expected may be."""
        sure = int(((self.label == self.expected) & self.safe)[rows].sum())
        return sure, sure + int((~self.safe[rows]).sum())


class Truth(Verdict):
    """The verdict on the fixture's own weights and rows, and G: flat gradient of the whole batch; (w, v): after N_STEPS steps on
    the whole batch."""

    def __init__(self, fx, dtype, jitter=None):
        super().__init__(fx, dtype, fx.Ws, fx.X, fx.Y, jitter)
        self.G = gradient(fx, dtype, fx.Ws, fx.X, fx.Y, jitter)
        w, v = fx.w.copy(), np.zeros_like(fx.w)
        for s in range(N_STEPS):
            w, v = oracle_step(fx, dtype, w, v, fx.X, fx.Y, jitter=jitter)
        self.w, self.v = w, v
        for a in vars(self).values():
            a.setflags(write=False)


class Restated:
    """The same quantities carried in float32: np_oracle's dtype=float32 forms, the loss as sum_j y_j (lse - z_j) in float32 --
    a plain restatement of what an f32 device computes."""

    def __init__(self, fx):
        f = np.float32
        Ws, X, Y = [W.astype(f) for W in fx.Ws], fx.X.astype(f), fx.Y.astype(f)
        a = (fx.inner, fx.out_kind, fx.last)
        Z, out = np_oracle.forward(Ws, X, *a, dtype=f)
        assert out.dtype == f
        self.out = out.astype(np.float64)
        if fx.out_kind == SCE:
            lse = np.log(np.exp(Z[-1]).sum(axis=1, keepdims=True, dtype=f), dtype=f)
            loss = (Y * (lse - Z[-1])).sum(axis=1, dtype=f)
        else:
            loss = (f(0.5) * (out - Y) ** 2).sum(axis=1, dtype=f)
        assert loss.dtype == f
        self.loss = loss.astype(np.float64)
        G = np_oracle.gradient(Ws, X, Y, *a, dtype=f)
        assert G.dtype == f
        self.G = G.astype(np.float64)
        w, v = fx.w.astype(f), np.zeros(fx.w.size, dtype=f)
        for s in range(N_STEPS):
            w, v = np_oracle.gradient_step(w, v, fx.dims, X, Y, STEP, MOMENTUM, *a, dtype=f)
        assert w.dtype == f and v.dtype == f
        self.w, self.v = w.astype(np.float64), v.astype(np.float64)


# ---- the budgets ------------------------------------------------------------------------------------------------------
def out_bound(fx, dtype, out_ref):
    if fx.out_kind == SCE or dtype == BF16:
        p = BUDGET[dtype]["p"]
    else:
        p = GENERAL_F32["p"]
    unbounded = fx.out_kind == GENERAL and fx.last in (IDENT, LEAKY, RELU)
    return p * (np.abs(out_ref).max() if unbounded else 1.0)


def loss_bound(fx, dtype, terms):
    """Per row, from the terms' absolute sum (Truth.terms)."""
    b = BUDGET[dtype] if fx.out_kind == SCE or dtype == BF16 else GENERAL_F32
    return b["l_rel"] * np.asarray(terms) + b["l_abs"]


def gradient_bounds(fx, dtype, G_ref):
    """Per layer: the budget times the layer's largest gradient entry, plus the absolute term."""
    b = BUDGET[dtype]
    return [b["g"] * np.abs(g).max() + b["g_abs"] for g in np_oracle.split(np.asarray(G_ref), fx.dims)]


def weight_bound(dtype, steps=N_STEPS):
    """W and V after `steps` steps: 2e-6 per step (f32), 2e-4 (bf16)."""
    return BUDGET[dtype]["w"] * (steps / N_STEPS if dtype == F32 else 1.0)


def loss_distance(fx, dtype, loss, t):
    """Largest per-row loss error in units of its bound; NaN / inf -> inf."""
    with np.errstate(all="ignore"):
        e = (np.abs(loss - t.loss) / loss_bound(fx, dtype, t.terms)).max()
    return e if np.isfinite(e) else np.inf


def gradient_distance(fx, dtype, G, G_ref):
    """Largest gradient error in units of its layer's bound."""
    e = 0.0
    for g, r, b in zip(np_oracle.split(np.asarray(G), fx.dims), np_oracle.split(np.asarray(G_ref), fx.dims), gradient_bounds(fx, dtype, G_ref)):
        e = max(e, float(np.abs(g - r).max() / b))
    return e


# ---- the faults the device tests must be able to see -------------------------------------------------------------------
def _one_hot_of_expected(Y):
    return np.eye(Y.shape[1])[expected_class(Y)]


def _pair(n):
    r = np.arange(n)
    return np.where((r ^ 1) < n, r ^ 1, r)


def _group_first(n):
    r = np.arange(n)
    return r - r % 16


# models that replace the expected rows: loss and gradient follow
TARGET_FAULTS = {
    "onehot": _one_hot_of_expected,                         # the label column instead of the row
    "clip": lambda Y: np.clip(Y, 0.0, 1.0),
    "ybf16": lambda Y: np_oracle.bf16_round(Y),
    "rowmix-pair": lambda Y: Y[_pair(len(Y))],              # the target row of row r ^ 1
    "rowmix-group": lambda Y: Y[_group_first(len(Y))],      # ... of the first row of the 16-row group
}
# models of the softmax loss expression alone
LOSS_FAULTS = ("sum1", "y>0", "y==1", "rowmix-sum")
SOFTMAX_FAULTS = LOSS_FAULTS + tuple(TARGET_FAULTS)
GENERAL_FAULTS = tuple(TARGET_FAULTS)


def faulty(fx, dtype, model):
    """(per-row loss, flat gradient or None) as the fault model forms them from the dtype's own logits."""
    t = fx.truth(dtype)
    Y = fx.Y
    if model in TARGET_FAULTS:
        Yf = TARGET_FAULTS[model](Y)
        return loss_rows(fx, t.Z, t.out, Yf)[0], gradient(fx, dtype, fx.Ws, fx.X, Yf)
    assert fx.out_kind == SCE
    zz = t.Z - t.Z.max(axis=1, keepdims=True)
    lse = np.log(np.exp(zz).sum(axis=1))
    if model == "sum1":                                     # right only when sum y = 1
        return lse - (Y * zz).sum(axis=1), None
    if model == "rowmix-sum":                               # sum y taken from row r ^ 1
        return Y.sum(axis=1)[_pair(len(Y))] * lse - (Y * zz).sum(axis=1), None
    keep = Y > 0 if model == "y>0" else Y == 1.0
    return np.where(keep, Y * (lse[:, None] - zz), 0.0).sum(axis=1), None


# ---- the sampled loops: the oracle stepping on the reference sampler's draws ----------------------------------------------
# train_sampled_held_out on T4: three points; every fifth draw is a refill of 5 rows (37 = 4 x 8 + 5).  The step is 0.1 so that the
# points differ by more than the bf16 loss budget (1 % of a loss sum of 110): 109.0, 113.8, 102.7
HELD = dict(iterations=12, batch=8, every=4, step=0.1)


def draws(oracle_mod, rows, sizes, seed=1):
    """The row indices NNT:143-168 hands out for batches of `sizes`, from a fresh Random(seed) sampler."""
    smp = oracle_mod.Sampler(rows, seed=seed)
    return [np.asarray(smp.sample(b)) for b in sizes]


def sampled_run(oracle_mod, fx, dtype, iterations, batch, seed=1, step=STEP, momentum=MOMENTUM):
    """[(w, v)] after every iteration of train_sampled (NNT:82-90) from the fixture's weights."""
    w, v, out = fx.w.copy(), np.zeros_like(fx.w), []
    for idx in draws(oracle_mod, fx.rows, [batch] * iterations, seed):
        w, v = oracle_step(fx, dtype, w, v, fx.X[idx], fx.Y[idx], step, momentum)
        out.append((w, v))
    return out


def held_out_curve(oracle_mod, fx, dtype):
    """(loss sums[P], their summed per-row bounds[P], (lo, hi) of the hits[P]) over the held-out rows at every point of HELD."""
    run = sampled_run(oracle_mod, fx, dtype, HELD["iterations"], HELD["batch"], step=HELD["step"])
    loss, bound, hits = [], [], []
    for i in range(HELD["every"] - 1, HELD["iterations"], HELD["every"]):
        t = Verdict(fx, dtype, np_oracle.split(run[i][0], fx.dims), fx.Xh, fx.Yh)
        loss.append(t.loss.sum())
        bound.append(loss_bound(fx, dtype, t.terms).sum())
        hits.append(t.hits_bounds())
    return np.array(loss), np.array(bound), hits
