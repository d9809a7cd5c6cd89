"""Fixtures of the group-evaluation tests (gnn_mlp_group_evaluate_range / _ensemble_range): the drawn nets, their inputs and
weights, and what the fp64 oracle says about them -- computed once per case and shared, never changed.

The shapes are the smallest at which the grouped forward kernel can still go wrong: ragged widths on both sides of 16, 64 and
1024, three to six layers, both output rules, row counts that are no multiple of 16, 32 or 64, and K = 16 (the whole pointer
table).  E7, E7b, E7g (more than 16 outputs, 1025 inputs) lie outside the kernel's plan: the member-after-member form, f32,
bf16 and General.  E9 / E9b have a hidden layer of more than 384 columns (several column passes of the kernel), E10 / E10b two
hidden layers so wide that the kernel takes tiles of 16 rows instead of 32.

Three weight scales are lower than first drawn, because a LONE bf16 member's propagate() already left the 5e-3 probability
budget against the fp64 oracle there (MI355X, single nets, no group call involved; the grouped kernel agrees with the lone path
to 6e-7): E1b at 0.5 gave 0.0084-0.0144 over its 16 members, 0.0048-0.0076 at 0.4, 0.0030-0.0063 at 0.35 and 0.0017-0.0033 at
0.31; E8 at 1.0 gave 0.021-0.036, at 0.5 0.0017-0.0023; E3b at 0.5 gave 0.0104-0.0128 (its mean over five members stayed
inside).  The error follows the largest logit, about 1e-3 per unit; the bf16 fixtures are scaled to logits of about 3.  The
budget stays; tests/test_group_eval_cpu.py holds for the lowered scales."""
import numpy as np

LEAKY, SIGMOID, TANH, RELU, IDENTITY = range(5)
SCE, GENERAL = 0, 1
F32, BF16 = 0, 1

#        name   dims                          kind     inner  last      dtype K   rows scale
_TABLE = [
    ("E1", [784, 300, 100, 10], SCE, LEAKY, IDENTITY, F32, 3, 150, 0.5),
    ("E1b", [784, 300, 100, 10], SCE, LEAKY, IDENTITY, BF16, 16, 150, 0.31),
    ("E2", [65, 33, 17, 10], SCE, TANH, IDENTITY, F32, 16, 131, 2.0),
    ("E3", [1023, 257, 128, 16], SCE, LEAKY, IDENTITY, F32, 2, 97, 0.5),
    ("E3b", [1023, 257, 128, 16], SCE, RELU, IDENTITY, BF16, 5, 97, 0.32),
    ("E4", [200, 90, 70, 50, 7], GENERAL, TANH, SIGMOID, F32, 5, 131, 1.0),
    ("E5", [129, 64, 48, 40, 31, 9], SCE, LEAKY, IDENTITY, F32, 5, 131, 1.0),
    ("E6", [300, 120, 12], GENERAL, TANH, SIGMOID, F32, 7, 70, 0.5),
    ("E6c", [300, 120, 12], SCE, TANH, IDENTITY, BF16, 3, 70, 0.5),
    ("E8", [200, 90, 70, 50, 7], SCE, LEAKY, IDENTITY, BF16, 4, 131, 0.5),
    ("E7", [1025, 374, 30], SCE, LEAKY, IDENTITY, F32, 2, 70, 0.5),
    # beyond the issue's table: the kernel's other code paths
    ("E9", [300, 520, 48, 12], SCE, LEAKY, IDENTITY, F32, 2, 50, 0.4),       # 33 column tiles: two passes (17 + 16), tiles of 32 rows
    ("E9b", [300, 520, 48, 12], SCE, LEAKY, IDENTITY, BF16, 3, 50, 0.38),
    ("E10", [60, 1000, 1000, 10], SCE, LEAKY, IDENTITY, F32, 2, 50, 0.5),    # two wide images: tiles of 16 rows, three passes of 21 tiles
    ("E10b", [60, 1000, 1000, 10], SCE, LEAKY, IDENTITY, BF16, 2, 50, 0.26),
    ("E7b", [1025, 374, 30], SCE, LEAKY, IDENTITY, BF16, 2, 70, 0.2),        # member after member, bf16
    ("E7g", [120, 50, 20], GENERAL, TANH, SIGMOID, F32, 3, 70, 1.0),         # member after member, General (20 outputs)
]


class Case:
    def __init__(self, name, dims, kind, inner, last, dtype, K, rows, scale):
        self.name, self.dims, self.kind, self.inner, self.last = name, dims, kind, inner, last
        self.dtype, self.K, self.rows, self.scale = dtype, K, rows, scale
        self.grouped = not name.startswith("E7")  # the grouped kernel applies (eval_launches == 2)

    def __repr__(self):
        return self.name


CASES = {row[0]: Case(*row) for row in _TABLE}
NAMES = [row[0] for row in _TABLE]


def inputs(case):
    """Centred, half-empty rows: positive inputs made untrained nets predict one class for every row."""
    d0 = case.dims[0]
    rng = np.random.default_rng(4000 + 100 * len(case.dims) + d0)
    return rng.standard_normal((case.rows, d0)) * (rng.random((case.rows, d0)) < 0.5)


def make_oracle(oracle_mod, case, seed=1):
    net = oracle_mod.OracleNet(case.dims, out_kind=case.kind, inner_act=case.inner, last_act=case.last, seed=seed)
    net.set_alloc_per_sample(0)
    return net


def member_weights(oracle_mod, case, k):
    """The f32-rounded Random(k + 1) draw (SCE:139-156) times the case's scale, as an f32 net holds it."""
    net = make_oracle(oracle_mod, case, seed=k + 1)
    w = net.get_weights().astype(np.float32).astype(np.float64) * case.scale
    net.close()
    return w.astype(np.float32).astype(np.float64)


def _top2_margin(a):
    s = np.sort(a, axis=1)
    return s[:, -1] - s[:, -2]


class Truth:
    """What the fp64 oracle says about a case with the given member weights.
    out[k], mean: outputs; label[k], ens_label: the reference's argmax; safe[k], ens_safe: rows whose top-2 margin exceeds
    the project's budgets (f32: 1e-3 on the logits / 1e-4 on a General net's outputs; bf16: 2e-3 max|Z| + 1e-3; the ensemble:
    the same dtype rule on the mean output); Y: the expected rows; loss[k]: calculateLoss per row."""

    def __init__(self, oracle_mod, case, weights, Y=None):
        self.case = case
        X = inputs(case)
        X = X.astype(np.float32).astype(np.float64)  # (the data set is f32 on the device)
        self.X = X
        K, n, d_out = len(weights), X.shape[0], case.dims[-1]
        nets = []
        self.out = np.empty((K, n, d_out))
        self.label = np.empty((K, n), dtype=np.int64)
        self.safe = np.empty((K, n), dtype=bool)
        for k in range(K):
            net = make_oracle(oracle_mod, case)
            net.set_weights(weights[k])
            nets.append(net)
            self.out[k] = net.propagate(X)
            self.label[k] = [oracle_mod.argmax_rule(r) for r in self.out[k]]
            z = net.logits(X) if case.kind == SCE else self.out[k]
            if case.dtype == BF16:
                self.safe[k] = _top2_margin(z) > 2e-3 * np.abs(z).max() + 1e-3
            else:
                self.safe[k] = _top2_margin(z) > (1e-3 if case.kind == SCE else 1e-4)
        self.mean = self.out.mean(axis=0)
        self.ens_label = np.array([oracle_mod.argmax_rule(r) for r in self.mean], dtype=np.int64)
        m = _top2_margin(self.mean)
        self.ens_safe = m > (2e-3 * np.abs(self.mean).max() + 1e-3 if case.dtype == BF16 else 1e-3)
        # expected rows: even rows the ensemble's own label (hits far from 0), odd rows (7 r) mod d_out
        cls = np.where(np.arange(n) % 2 == 0, self.ens_label, (7 * np.arange(n)) % d_out)
        if Y is not None:  # (rows already uploaded: one-hot)
            cls = np.asarray(Y).argmax(axis=1)
        self.Y = np.eye(d_out)[cls]
        self.expected = cls
        self.loss = np.stack([np.atleast_1d(net.calculate_loss(X, self.Y)) for net in nets])
        for net in nets:
            net.close()

    def hits_bounds(self, label, safe, lo=0, hi=None):
        """[hits on safe rows, the same + unsafe rows] over rows [lo, hi)."""
        hi = self.X.shape[0] if hi is None else hi
        sl = slice(lo, hi)
        sure = int(((label[sl] == self.expected[sl]) & safe[sl]).sum())
        return sure, sure + int((~safe[sl]).sum())


_truth = {}


def truth(oracle_mod, name):
    """The oracle's verdict on a case with its own weights: computed once, shared by every test, left unchanged."""
    if name not in _truth:
        case = CASES[name]
        _truth[name] = Truth(oracle_mod, case, [member_weights(oracle_mod, case, k) for k in range(case.K)])
    return _truth[name]
