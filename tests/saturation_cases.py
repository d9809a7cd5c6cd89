"""Fixtures of the saturated-logit tests (tests/test_saturation_cpu.py pins them and shows that the fault models below leave
the budgets on them; tests/test_saturation_gpu.py runs them through every output head on the device): small nets whose
softmax rows lie in DIFFERENT regimes within one 4-row block and one 16-lane row -- all logits near +150, all near -150, all
near 0 -- or whose logits are spread over +-300.  The rest of the suite keeps every logit within a band in which any finite
"maximum" gives the same probabilities; here only the row's own maximum does.  No GPU code: numpy and tests/np_oracle.py.

SHIFT fixtures.  Softmax nets have no bias, so a per-row constant rides on two dedicated units, u+ = 0 and u- = 1: in every
layer below the last they connect only to the same unit of the layer before (chain weight > 0, every other weight into and out
of them 0); input column u+ is ON for high rows, u- for low rows, both OFF for neutral rows; rows u+ / u- of the last layer hold
+c / -c in EVERY column, c = 150 / (kappa_on - kappa_off) with the kappas read from the fp64 oracle's last hidden activations.
Row classes cycle neutral / high / low by row % 3.  Every other weight is the Random(1) draw scaled as
tests/test_gemm_edges_gpu.py::_scaled_weights does; the input rows are picked from a seeded draw of candidates by their top-2
logit margin (the shift does not change it), so that labels can be compared on nearly every row.

SPREAD fixtures.  No chain: the last layer is scaled (one boosted column where there are more than 16) and the rows are picked
from a seeded draw of candidates so that EVERY row has an fp64 top-2 gap >= 110, a logit range <= 300 and max |z| <= 300.  Even
rows expect the argmax class (p == 1.0f), odd rows the class of the LOWEST logit (p underflows to 0 in f32; loss 110 .. 300).

GENERAL fixtures.  The shift construction on GeneralNeuralNet (out_kind 1) with each of the five last activations.

Measured on the CPU (tests/test_saturation_cpu.py prints them), in units of the probability / loss budgets:
  correct f32 head on fp64 logits, and on logits from f32-rounded last hidden activations .. <= 0.025 on every fixture
  bf16 oracle under jitter 1e-6, four seeds, the f32 head on top ........................... <= 0.16 (S4s; else <= 0.04)
  so no spread fixture is dropped for bf16.
The one known amplification: into the chain units delta_{L-2}[u+-] = c * sum_col(p - y), 0 in exact arithmetic and c x f32
roundings on the device (of p, and of a sum whose partial sums pass +-c).  CHAIN_NOISE_SEEN holds chain_noise() -- the largest
such gradient entry -- per fixture as measured when the fixtures were drawn; the GPU test recomputes it and widens ONLY the
columns u+ / u- of the layers below the last, by 4 x it.
"""
import numpy as np

from tests import np_oracle

LEAKY, SIGMOID, TANH, RELU, IDENT = range(5)
SCE, GENERAL = 0, 1
F32, BF16 = 0, 1
UP, UM = 0, 1                        # the chain units u+ and u-
NEUTRAL, HIGH, LOW = 0, 1, 2         # row classes, row % 3
SHIFT = 150.0
STEP, MOMENTUM, N_STEPS = 0.0125, 0.9, 2
JITTER, JITTER_SEEDS = 1e-6, (1, 2, 3, 4)
BUDGET = {   # the suite's own: probabilities, loss (relative + absolute), gradients (x max |G_l| + absolute), W and V
    F32: dict(p=2e-4, l_rel=2e-4, l_abs=2e-4, g=3e-5, g_abs=1e-9, w=2e-6 * N_STEPS),
    BF16: dict(p=5e-3, l_rel=1e-2, l_abs=1e-3, g=4e-3, g_abs=1e-7, w=2e-4),
}
# (ON input, OFF input, chain weight).  Sigmoid has no off state of 0 (ON 6, OFF -6: c = 395 behind one hidden layer, 1 233
# behind two -- with OFF 0 it was 3 621, and the f32 sums of terms c x kappa = +-2 900 then round at 1.2e-4 per addition, above
# the gradient budget by themselves); tanh saturates: both need c >= 150.  Leaky ReLU and
# ReLU: an OFF state of 0 would park the chain units exactly on the kink, where after the first update a pre-activation of
# +-1e-9 (the noise below, of either sign) decides between two derivatives -- both states lie on the positive side.
CHAIN = {LEAKY: (1.5, 0.5, 1.0), RELU: (1.5, 0.5, 1.0), IDENT: (1.0, 0.0, 1.0), TANH: (3.0, 0.0, 2.0), SIGMOID: (6.0, -6.0, 2.0)}

#         name        kind      dims                    out      inner    last   rows
_TABLE = [
    ("S3",      "shift",  [20, 12, 10],            SCE,     LEAKY,   IDENT, 21),
    ("S4",      "shift",  [20, 12, 8, 10],         SCE,     TANH,    IDENT, 37),
    ("S4s",     "shift",  [20, 12, 8, 10],         SCE,     SIGMOID, IDENT, 21),   # two sigmoid hidden layers: c = 1233
    ("S16",     "shift",  [20, 12, 8, 16],         SCE,     RELU,    IDENT, 37),   # 16 outputs: no padding column
    ("S132",    "shift",  [20, 132, 10],           SCE,     LEAKY,   IDENT, 21),   # last hidden layer > 128: middle4's register head
    ("S17",     "shift",  [20, 12, 17],            SCE,     SIGMOID, IDENT, 37),   # more than 16 outputs: middle4's general head
    ("S40",     "shift",  [20, 12, 9, 8, 7, 40],   SCE,     IDENT,   IDENT, 21),
    ("S1100",   "shift",  [40, 24, 1100],          SCE,     LEAKY,   IDENT, 6),    # the output kernel's three-pass form
    ("P4",      "spread", [20, 12, 8, 10],         SCE,     LEAKY,   IDENT, 37),
    ("P16",     "spread", [20, 12, 8, 16],         SCE,     TANH,    IDENT, 21),
    ("P132",    "spread", [20, 132, 10],           SCE,     TANH,    IDENT, 21),
    ("P17",     "spread", [20, 12, 17],            SCE,     LEAKY,   IDENT, 21),
    ("P1100",   "spread", [40, 24, 1100],          SCE,     LEAKY,   IDENT, 6),
    ("G_ident", "shift",  [20, 12, 8, 10],         GENERAL, TANH,    IDENT, 21),
    ("G_leaky", "shift",  [20, 12, 8, 10],         GENERAL, TANH,    LEAKY, 21),
    ("G_relu",  "shift",  [20, 12, 8, 10],         GENERAL, LEAKY,   RELU, 21),
    ("G_sigm",  "shift",  [20, 12, 8, 10],         GENERAL, LEAKY,   SIGMOID, 37),
    ("G_tanh",  "shift",  [20, 12, 8, 10],         GENERAL, RELU,    TANH, 21),
    ("G17",     "shift",  [20, 12, 17],            GENERAL, TANH,    IDENT, 21),   # more than 16 outputs
]
NAMES = [r[0] for r in _TABLE]
SOFTMAX_SHIFT = [r[0] for r in _TABLE if r[1] == "shift" and r[3] == SCE]
SPREAD = [r[0] for r in _TABLE if r[1] == "spread"]
GENERAL_NAMES = [r[0] for r in _TABLE if r[3] == GENERAL]

# chain_noise() as measured when the fixtures were drawn: largest |G - G_fp64| over the chain columns, (f32, bf16)
CHAIN_NOISE_SEEN = {
    "S3": (6.2e-05, 0.0017),      # c = 150
    "S4": (0.00011, 0.0024),      # c = 156.5
    "S4s": (5.8e-05, 0.15),       # c = 1232
    "S16": (0.00013, 0.034),      # c = 150
    "S132": (3.7e-05, 0.00024),   # c = 150
    "S17": (4.2e-05, 0.0),        # c = 395.7 (bf16: every product and partial sum is exact)
    "S40": (0.00023, 0.003),      # c = 150
    "S1100": (0.00011, 0.0059),   # c = 150
}


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def _scaled_draw(oracle_mod, dims, out_kind, inner, last, seed=1, gain=2.0):
    """The f32 Random(seed) draw, each layer scaled to a standard deviation of gain / sqrt(fan-in)."""
    net = oracle_mod.OracleNet(dims, out_kind=out_kind, inner_act=inner, last_act=last, seed=seed)
    w = f32(net.get_weights())
    net.close()
    Ws = [W.copy() for W in np_oracle.split(w, dims)]
    for l, W in enumerate(Ws):
        W *= gain / (np.sqrt(dims[l]) * np.sqrt(1.0 / 12))
    return Ws


def _candidates(seed, n, d0):
    rng = np.random.default_rng(seed)
    return f32(rng.random((n, d0)) * (rng.random((n, d0)) < 0.5)), rng


def _top2_gap(z):
    s = np.sort(z, axis=1)
    return s[:, -1] - s[:, -2]


class Fixture:
    """One net, its weights (f32-exact, flat `w` and per layer `Ws`), rows X (f32-exact), expected rows Y, row classes `cls`."""

    def __init__(self, oracle_mod, name, kind, dims, out_kind, inner, last, rows, seed=1, like=None):
        """seed: the Random(seed) draw.  like: another member of a net group -- its rows, expected rows and last-layer scale."""
        self.name, self.kind, self.dims, self.out_kind, self.inner, self.last, self.rows = name, kind, dims, out_kind, inner, last, rows
        self.c = 0.0
        d_out, Lm = dims[-1], len(dims) - 1
        Ws = _scaled_draw(oracle_mod, dims, out_kind, inner, last, seed)
        X, rng = _candidates(9000 + 10 * len(dims) + d_out, 6000, dims[0])
        if kind == "shift":
            on, off, wc = CHAIN[inner]
            for l in range(Lm - 1):
                for u in (UP, UM):
                    Ws[l][u, :] = 0.0
                    Ws[l][:, u] = 0.0
                    Ws[l][u, u] = wc
            Ws[Lm - 1][(UP, UM), :] = 0.0
            X[:, (UP, UM)] = off
            # rows whose labels can be compared: a top-2 margin of the unshifted logits above every budget of the margin rule
            Z, _ = np_oracle.forward(Ws, X, inner, out_kind, last)
            keep = np.flatnonzero(_top2_gap(Z[-1]) > 0.45)[:rows]
            assert keep.size == rows, "fixture %s: too few candidate rows" % name
            X = X[keep] if like is None else like.X.copy()
            self.cls = np.arange(rows) % 3
            X[self.cls == HIGH, UP] = on
            X[self.cls == LOW, UM] = on
            # c from the oracle's own last hidden activations (row 1 is high, row 0 neutral)
            Z, _ = np_oracle.forward(Ws, X, inner, out_kind, last)
            kappa = np_oracle.act(inner, Z[Lm - 1])[:, UP]
            self.c = float(np.float32(SHIFT / (kappa[1] - kappa[0])))
            Ws[Lm - 1][UP, :] = self.c
            Ws[Lm - 1][UM, :] = -self.c
            self.Y = np.eye(d_out)[rng.integers(0, d_out, rows)] if like is None else like.Y
        elif like is not None:
            Ws[Lm - 1] = f32(Ws[Lm - 1] * like.last_scale)
            X, self.Y, self.cls = like.X.copy(), like.Y, like.cls
        else:
            boosted = d_out > 16   # (the top-2 gap of hundreds of like columns is a small fraction of their range)
            Z, _ = np_oracle.forward(Ws, X, inner, out_kind, last)
            col = np.ones(d_out)
            if boosted:
                col[:] = 30.0 / np.abs(Z[-1]).max()
                col[3] = 250.0 / np.abs(Z[-1][:, 3]).max()
            keep = None
            for s in (1.0 if boosted else 120.0 / Z[-1].std()) * np.array([1.0, 1.15, 1.3, 1.5, 0.85]):
                W_last = f32(Ws[Lm - 1] * col * s)
                z = np_oracle.act(inner, Z[Lm - 1]) @ W_last
                ok = (np.abs(z).max(axis=1) <= 300.0) & (_top2_gap(z) >= 112.0) & (z.max(axis=1) - z.min(axis=1) <= 298.0)
                if ok.sum() >= rows:
                    keep = np.flatnonzero(ok)[:rows]
                    break
            assert keep is not None, "fixture %s: too few candidate rows" % name
            Ws[Lm - 1] = W_last
            self.last_scale = col * s
            X = X[keep]
            self.cls = np.full(rows, -1)
            z = z[keep]
            want = np.where(np.arange(rows) % 2 == 0, z.argmax(axis=1), z.argmin(axis=1))
            self.Y = np.eye(d_out)[want]
        self.Ws = [f32(W) for W in Ws]
        self.w = np.concatenate([W.ravel() for W in self.Ws])
        self.X = X
        # the columns whose gradient, weight and momentum entries carry c x (the f32 rounding of sum(p - y)): per layer
        self.chain_cols = {l: (UP, UM) for l in range(Lm - 1)} if kind == "shift" and out_kind == SCE else {}

    def __repr__(self):
        return self.name

    # ---- the oracles' verdicts (computed on demand, cached, never changed) ----
    def truth(self, dtype):
        key = "_truth%d" % dtype
        if not hasattr(self, key):
            setattr(self, key, Truth(self, dtype))
        return getattr(self, key)


class Truth:
    """Z: logits; out: probabilities / outputs; loss per row; G: flat gradient of the whole batch; (w, v): after N_STEPS steps
    on the whole batch; label (the reference's `>=` argmax: ties to the highest index) and safe rows (the project's margin rule)."""

    def __init__(self, fx, dtype, jitter=None, forward_only=False):
        bf = dtype == BF16
        a = (fx.inner, fx.out_kind, fx.last)
        if bf:
            Z, _, out = np_oracle.forward_bf16(fx.Ws, fx.X, *a, jitter=jitter)
        else:
            Z, _ = np_oracle.forward(fx.Ws, fx.X, *a)
            out = None
        self.Z = Z[-1]
        if fx.out_kind == SCE:
            zz = self.Z - self.Z.max(axis=1, keepdims=True)   # (the same numbers as the un-normalised form, without its 1e130s)
            lse = np.log(np.exp(zz).sum(axis=1, keepdims=True))
            self.out = np.exp(zz - lse)
            self.loss = (fx.Y * (lse - zz)).sum(axis=1)
        else:
            self.out = np_oracle.act(fx.last, self.Z) if out is None else out
            self.loss = (0.5 * (self.out - fx.Y) ** 2).sum(axis=1)
        key = self.Z if fx.out_kind == SCE else self.out
        self.label = np.array([int(np.flatnonzero(r >= r.max())[-1]) for r in key])
        margin = _top2_gap(key)
        if fx.out_kind == SCE:
            self.safe = margin > (2e-3 * np.abs(self.Z).max() + 1e-3 if bf else 1e-3)
        else:
            self.safe = margin > (2e-3 * np.abs(self.out).max() + 1e-3 if bf else 1e-4 * max(1.0, np.abs(self.out).max()))
        if jitter is not None or forward_only:
            return
        if bf:
            self.G = np_oracle.gradient_bf16(fx.Ws, fx.X, fx.Y, *a)
        else:
            self.G = np_oracle.gradient(fx.Ws, fx.X, fx.Y, *a)
        step = step_size(fx, self.G)
        w, v = fx.w.copy(), np.zeros_like(fx.w)
        for _ in range(N_STEPS):
            if bf:
                w, v = np_oracle.gradient_step_bf16(w, v, fx.dims, fx.X, fx.Y, step, MOMENTUM, *a)
            else:
                w, v = np_oracle.gradient_step(w, v, fx.dims, fx.X, fx.Y, step, MOMENTUM, *a)
        self.w, self.v, self.step = w, v, step


def step_size(fx, G):
    """STEP for softmax nets.  A General net with outputs of +-150 has gradients of 1e4 and more: the step is the power of two
    that keeps the largest update of a step below STEP (weights of order one stay of order one, and the absolute W budget keeps
    its meaning)."""
    if fx.out_kind == SCE:
        return STEP
    g = np.abs(G).max() / fx.rows
    return STEP if g <= 1.0 else STEP * 2.0 ** -np.ceil(np.log2(g))


_fixtures = {}


def fixture(oracle_mod, name, seed=1):
    """The fixture (seed 1), or the net of Random(seed) on the same rows: a further member of a net group."""
    if (name, seed) not in _fixtures:
        row = next(r for r in _TABLE if r[0] == name)
        _fixtures[(name, seed)] = Fixture(oracle_mod, *row) if seed == 1 else Fixture(oracle_mod, *row, seed=seed, like=fixture(oracle_mod, name))
    return _fixtures[(name, seed)]


# ---- numpy-f32 heads: the correct one and the faults the device tests must be able to see ------------------------------
def _softmax_head(Z, Y, mx):
    z = np.asarray(Z, dtype=np.float32)
    mx = np.asarray(mx, dtype=np.float32).reshape(-1, 1)
    with np.errstate(all="ignore"):
        e = np.exp(z - mx, dtype=np.float32)
        s = e.sum(axis=1, keepdims=True, dtype=np.float32)
        p = e * (np.float32(1.0) / s)
        lse = mx + np.log(s, dtype=np.float32)
        loss = np.where(Y != 0, Y.astype(np.float32) * (lse - z), np.float32(0.0)).sum(axis=1, dtype=np.float32)
    return p.astype(np.float64), loss.astype(np.float64)


def _group_max(Z, rows_per_group):
    z = np.asarray(Z, dtype=np.float32)
    mx = z.max(axis=1)
    out = mx.copy()
    for g in range(0, z.shape[0], rows_per_group):
        out[g:g + rows_per_group] = mx[g:g + rows_per_group].max()
    return out


def head_correct(Z, Y):
    return _softmax_head(Z, Y, np.asarray(Z, dtype=np.float32).max(axis=1))


def head_f1_no_subtraction(Z, Y):
    return _softmax_head(Z, Y, np.zeros(len(Z)))


def head_f2_pad_column(Z, Y):
    """The maximum includes one padding column, which holds an exact 0."""
    return _softmax_head(Z, Y, np.maximum(np.asarray(Z, dtype=np.float32).max(axis=1), 0.0))


def head_f3_block_max(Z, Y):
    """The maximum shared by the 4 rows of a row block."""
    return _softmax_head(Z, Y, _group_max(Z, 4))


def head_f3w_dpp_row_max(Z, Y):
    """The maximum shared by 16 rows."""
    return _softmax_head(Z, Y, _group_max(Z, 16))


def head_f4_log_p(Z, Y):
    """The loss as -log of the f32 probability."""
    p, _ = head_correct(Z, Y)
    with np.errstate(all="ignore"):
        lp = -np.log(p.astype(np.float32), dtype=np.float32)
        return p, np.where(Y != 0, Y.astype(np.float32) * lp, np.float32(0.0)).sum(axis=1, dtype=np.float32).astype(np.float64)


def head_f5_max_zero(Z, Y):
    """The maximum left at a stale value: the row before's (what a register or an LDS slot written one trip late holds), and
    the initial 0 for the first row -- a high row after a neutral one overflows, a low row after a high one underflows."""
    mx = np.asarray(Z, dtype=np.float32).max(axis=1)
    return _softmax_head(Z, Y, np.r_[np.float32(0.0), mx[:-1]])


def sigmoid_f32(z):
    z = np.asarray(z, dtype=np.float32)
    with np.errstate(all="ignore"):
        return (np.float32(1.0) / (np.float32(1.0) + np.exp(-z, dtype=np.float32))).astype(np.float64)


def sigmoid_f6(z):
    """Sigmoid as e^z / (1 + e^z)."""
    z = np.asarray(z, dtype=np.float32)
    with np.errstate(all="ignore"):
        e = np.exp(z, dtype=np.float32)
        return (e / (np.float32(1.0) + e)).astype(np.float64)


SHIFT_FAULTS = {"F1": head_f1_no_subtraction, "F2": head_f2_pad_column, "F3": head_f3_block_max, "F3'": head_f3w_dpp_row_max,
                "F5": head_f5_max_zero}


def in_budget(p, loss, t, dtype, fraction=1.0):
    """(largest probability error, largest loss error over its bound) in units of `fraction` of the budgets; NaN / inf -> inf."""
    b = BUDGET[dtype]
    with np.errstate(all="ignore"):
        ep = np.abs(p - t.out).max() / (fraction * b["p"])
        el = (np.abs(loss - t.loss) / (fraction * (b["l_rel"] * np.abs(t.loss) + b["l_abs"]))).max()
    ep = ep if np.isfinite(ep) else np.inf
    el = el if np.isfinite(el) else np.inf
    return ep, el


# ---- the one known amplification -------------------------------------------------------------------------------------
def chain_noise(fx, dtype):
    """Into the chain units delta_{L-2}[u+-] = c * sum_col(p - y): 0 in exact arithmetic, c x an f32 rounding on the device.
    Measured: the gradient with the CORRECT f32 head's p - y (bf16: under jitter, four seeds) against the oracle's, largest
    difference per layer over the chain columns -- {layer: value}.  Only those columns may be widened, by 4 x this."""
    if not fx.chain_cols:
        return {}
    t = fx.truth(dtype)
    Gs = []
    if dtype == F32:
        p32, _ = head_correct(t.Z, fx.Y)
        d32 = (p32.astype(np.float32) - fx.Y.astype(np.float32)).astype(np.float64)
        Gs += [_gradient_from_delta(fx, d32, order=o) for o in range(N_ORDERS)]
    else:
        for seed in JITTER_SEEDS:
            Gs.append(np_oracle.gradient_bf16(fx.Ws, fx.X, fx.Y, fx.inner, fx.out_kind, fx.last,
                                              jitter=(JITTER, np.random.default_rng(seed))))
        p32, _ = head_correct(t.Z, fx.Y)   # and the f32 head on the bf16 path's logits
        d32 = (p32.astype(np.float32) - fx.Y.astype(np.float32)).astype(np.float64)
        Gs += [_gradient_from_delta(fx, d32, bf=True, order=o) for o in range(N_ORDERS)]
    ref = np_oracle.split(t.G, fx.dims)
    noise = {}
    for l, cols in fx.chain_cols.items():
        noise[l] = max(float(np.abs(np_oracle.split(G, fx.dims)[l][:, cols] - ref[l][:, cols]).max()) for G in Gs)
    return noise


N_ORDERS = 3


def _dot32(D, w, order):
    """sum_col D[:, col] * w[col] added up in f32, in one of three orders: ascending columns, descending, four interleaved
    partial sums (columns k, k + 4, ..: how the row tails split a product).  The partial sums pass +-c (the expected class's
    -c y), so every addition rounds at spacing(c) / 2 -- the rounding the device's backward product into the chain units has."""
    P = D.astype(np.float32) * w.astype(np.float32)
    if order == 0:
        return np.cumsum(P, axis=1, dtype=np.float32)[:, -1].astype(np.float64)
    if order == 1:
        return np.cumsum(P[:, ::-1], axis=1, dtype=np.float32)[:, -1].astype(np.float64)
    parts = [np.cumsum(P[:, j::4], axis=1, dtype=np.float32)[:, -1] for j in range(4)]
    return ((parts[0] + parts[1]) + (parts[2] + parts[3])).astype(np.float64)


def _gradient_from_delta(fx, D, bf=False, order=0):
    """np_oracle.gradient / gradient_bf16 with the last layer's delta given and the product into the chain units added in f32."""
    q = np_oracle.bf16_round if bf else (lambda x: x)
    if bf:
        Z, A, _ = np_oracle.forward_bf16(fx.Ws, fx.X, fx.inner, fx.out_kind, fx.last)
        acts = [q(a) for a in A]
    else:
        Z, _ = np_oracle.forward(fx.Ws, fx.X, fx.inner, fx.out_kind, fx.last)
        acts = [np_oracle.act(fx.inner, z) for z in Z[:-1]]
    G = [None] * len(fx.Ws)
    for l in range(len(fx.Ws) - 1, -1, -1):
        Dq = q(D)
        G[l] = acts[l].T @ Dq
        if l >= 1:
            Dn = Dq @ q(fx.Ws[l]).T
            if l == len(fx.Ws) - 1:
                for u in (UP, UM):
                    Dn[:, u] = _dot32(Dq, q(fx.Ws[l])[u], order)
            D = Dn * np_oracle.act_prime(fx.inner, Z[l])
    return np.concatenate([g.ravel() for g in G])


def gradient_bounds(fx, dtype, G_ref):
    """Per layer an array of the element-wise gradient bounds: the layer budget, plus 4 x chain_noise on the chain columns."""
    b, noise, out = BUDGET[dtype], chain_noise(fx, dtype), []
    for l, g in enumerate(np_oracle.split(np.asarray(G_ref), fx.dims)):
        tol = np.full(g.shape, b["g"] * np.abs(g).max() + b["g_abs"])
        if l in fx.chain_cols:
            tol[:, fx.chain_cols[l]] += 4.0 * noise[l]
        out.append(tol)
    return out


BIG_W = 16.0


def weight_bounds(fx, dtype, w_ref, step, masters=True):
    """Per layer the element-wise bounds of W and V after N_STEPS steps.  The budget; on the chain columns plus what 4 x the
    gradient noise becomes in N_STEPS = 2 updates (v1 = s g1, v2 = s g2 + mu v1, w2 = w0 - v1 - v2: at most (2 + mu) s x noise);
    and on the entries of the LAST layer with |w| >= BIG_W = 16 -- rows u+ / u- of a shift fixture (+-c, 150 .. 1 233: f32 masters
    spaced 1.5e-5 .. 1.2e-4 apart, above the budget itself) and most of a spread fixture's scaled last layer -- half a spacing of
    the value per step: what storing the exact result in an f32 master costs (the W budget of 2e-6 per step presumes weights of
    order one, spaced 1.2e-7; V, the update itself, keeps the plain budget everywhere but on the chain columns)."""
    b, noise, out = BUDGET[dtype], chain_noise(fx, dtype), []
    Lm = len(fx.dims) - 1
    for l, w in enumerate(np_oracle.split(np.asarray(w_ref), fx.dims)):
        tol = np.full(w.shape, b["w"])
        if l in fx.chain_cols:
            tol[:, fx.chain_cols[l]] += 4.0 * noise[l] * (2.0 + MOMENTUM) * step / fx.rows
        if l == Lm - 1 and masters:
            big = np.abs(w) >= BIG_W
            tol[big] += N_STEPS * 0.5 * np.spacing(np.abs(w[big]).astype(np.float32)).astype(np.float64)
        out.append(tol)
    return out


def widened_entries(fx, w_ref):
    """{layer: number of entries whose bound differs from the layer's budget}: gradient / momentum (the chain columns: at most
    this many, none where the measured noise is 0), weights (the same, and in the last layer exactly the entries of the stepped
    reference weights w_ref with |w| >= BIG_W -- in a shift fixture rows u+ / u-)."""
    Lm = len(fx.dims) - 1
    g = {l: len(c) * fx.dims[l] for l, c in fx.chain_cols.items()}
    w = dict(g)
    w[Lm - 1] = int((np.abs(np_oracle.split(np.asarray(w_ref), fx.dims)[Lm - 1]) >= BIG_W).sum())
    return g, w


def loss_at(fx, dtype, w):
    """calculateLoss per row with the flat weights w in place of the fixture's (the dtype's oracle)."""
    import copy
    other = copy.copy(fx)
    other.Ws = np_oracle.split(np.asarray(w, dtype=np.float64), fx.dims)
    return Truth(other, dtype, forward_only=True).loss


def oracle_step(fx, dtype, w, v, idx, step):
    """One gradientStep on rows idx."""
    fn = np_oracle.gradient_step_bf16 if dtype == BF16 else np_oracle.gradient_step
    return fn(w, v, fx.dims, fx.X[idx], fx.Y[idx], step, MOMENTUM, fx.inner, fx.out_kind, fx.last)
