"""Integrated gradients (gnn_mlp_integrated_gradients_set_range, gnn_amd.integrated_gradients): the fp64 model, its float32
restatement, the budgets, the fault models and the fixtures of tests/test_intgrad_cpu.py and tests/test_intgrad_gpu.py.  No tests
here.

x0 is the row, b_f the float32 baseline, m the number of path points, g(a) the input gradient at a (tests/adversarial_cases.py:
gradient).  In f32, every operation rounded on its own:

    alpha_k = float32((k + 0.5) / m)             midpoints, formed in double and rounded once
    d    = x0 - b_f
    a_k  = b_f + alpha_k * d
    S_0  = g(a_0);   S_k = S_{k-1} + g(a_k)
    IG   = d * (S_{m-1} / float32(m))

The model takes the path points and d as the FLOAT32 values above (rows are float32 values on the device) and carries g, the sum,
the division and the product in fp64.  Nothing here depends on a sign: no cell is excluded from any comparison.

The element budget: |d| x the mean over k of tests/input_gradient_cases.py's budget of g(a_k) (F32_RTOL max|g(a_k)| + F32_ATOL
over the fixture's rows; bf16: BF16_RTOL / BF16_ATOL), plus 2^-22 |IG| for the roundings of the sum, the division and the product.

The fixtures, their weights (SCALE = 0.2 times the reference net's Random(1) draw) and rows are tests/adversarial_cases.py's."""
import collections
import functools

import numpy as np

from tests import adversarial_cases as ac
from tests import np_oracle as npo

STEPS = 8
BASELINES = (0.0, 0.25)       # 0.25: d is negative on many cells, and more hidden units change side along the path
ONE_STEP = ("ident", 1, 0.25)  # the one case with steps = 1: S is never read or written, the first step is the last
MORE_STEPS = 32               # what m buys: the gap at 32 points against 8
CASES = ac.CASES
BF16_CASES = ac.BF16_CASES
ALL = [(c.name, False) for c in CASES] + [(c.name, True) for c in BF16_CASES]


def f32(x):
    return np.float32(x)


def alphas(m, rule="mid"):
    """float32 path parameters; rule "left": the left-endpoint rule k / m (a fault)"""
    off = 0.5 if rule == "mid" else 0.0
    return [f32((k + off) / m) for k in range(m)]


def points(X, baseline, m, rule="mid"):
    """(d, [a_0 .. a_{m-1}]) in float32, as defined"""
    x0, b = np.asarray(X, dtype=np.float32), f32(baseline)
    d = x0 - b
    return d, [b + al * d for al in alphas(m, rule)]


Model = collections.namedtuple("Model", "ig d gs budget")     # ig: fp64 (n, d0); gs[k]: g at a_k; budget: (n, d0)


def element_budget(d, gs, ig, bf16=False):
    mean = float(np.mean([ac.budget(g, bf16) for g in gs]))
    return np.abs(np.asarray(d, dtype=np.float64)) * mean + 2.0 ** -22 * np.abs(ig)


def model(Ws, X, Y, inner, steps=STEPS, baseline=0.0, bf16=False, fault=None, max_batch=None):
    """fp64 on the float32 points.  `fault` names one way to get the device route wrong; max_batch: the block size of the range
    call (the stale-sum fault needs it)."""
    m = int(steps)
    d, pts = points(X, baseline, m, "left" if fault == "left_endpoint" else "mid")
    d64 = d.astype(np.float64)
    gs = []
    for a in pts:
        a64 = a.astype(np.float64)
        if fault == "no_fprime":          # f' left out of the l = 0 factor
            gs.append(ac.product(Ws, a64, Y, inner))
        else:
            gs.append(ac.gradient(Ws, a64, Y, inner, bf16))
    terms = gs[:-1] if fault == "drop_last" and m > 1 else gs
    S = np.sum(terms, axis=0)
    if fault == "stale_sum" and m > 1:    # S_0 = (what the previous block left: its S_{m-2}) + g(a_0), row for row
        mb = max_batch or len(X)
        left = np.sum(gs[:-1], axis=0)
        for off in range(mb, len(X), mb):
            B = min(mb, len(X) - off)
            S[off:off + B] += left[off - mb:off - mb + B]
    if fault == "d_from_point":           # d taken from the staging point of the last step, not from the origin
        d64 = (pts[-1] - f32(baseline)).astype(np.float64)
    ig = d64 * S if fault == "no_mean" else d64 * (S / float(m))
    return Model(ig, d, gs, None)


FAULTS = ("left_endpoint", "no_mean", "drop_last", "d_from_point", "no_fprime", "stale_sum")


def restatement(Ws, X, Y, inner, steps=STEPS, baseline=0.0, bf16=False):
    """the definition carried in float32: g from the float32 forms of the gradient (bf16: the bf16 model's g rounded to float32),
    the sum in step order, the division, the product"""
    m = int(steps)
    d, pts = points(X, baseline, m)
    S = None
    for a in pts:
        a64 = a.astype(np.float64)
        g = ac.gradient(Ws, a64, Y, inner, True).astype(np.float32) if bf16 else ac.gradient_f32(Ws, a64, Y, inner)
        assert g.dtype == np.float32
        S = g if S is None else S + g
    out = d * (S / f32(m))
    assert out.dtype == np.float32
    return out


@functools.lru_cache(maxsize=None)
def _reference(oracle_mod, name, bf16, baseline, steps, held):
    c = ac.BY_NAME[name]
    X, Y = ac.held_rows(c) if held else ac.rows(c)
    mo = model(ac.weights(oracle_mod, c), X, Y, c.inner, steps, baseline, bf16)
    mo = mo._replace(budget=element_budget(mo.d, mo.gs, mo.ig, bf16))
    for a in (mo.ig, mo.d, mo.budget) + tuple(mo.gs):
        a.setflags(write=False)
    return mo


def reference(oracle_mod, case, baseline=0.0, bf16=False, steps=STEPS, held=False):
    """the model on the fixture's rows with its element budget, computed once and shared (read-only)"""
    return _reference(oracle_mod, case.name, bool(bf16), float(baseline), int(steps), bool(held))


# ---- completeness: sum_i IG_i = L(x) - L(baseline) ---------------------------------------------------------------------------------
def completeness_gap(Ws, X, Y, inner, ig, baseline):
    """per row, fp64: the attributions summed minus the loss difference between the float32 row and the baseline row"""
    x0 = np.asarray(X, dtype=np.float32).astype(np.float64)
    base = np.full(x0.shape, float(f32(baseline)))
    return np.asarray(ig, dtype=np.float64).sum(axis=1) - (npo.loss(Ws, x0, Y, inner) - npo.loss(Ws, base, Y, inner))


@functools.lru_cache(maxsize=None)
def _gap(oracle_mod, name, baseline, steps, rule):
    c = ac.BY_NAME[name]
    X, Y = ac.rows(c)
    Ws = ac.weights(oracle_mod, c)
    ig = reference(oracle_mod, c, baseline, False, steps).ig if rule == "mid" else model(Ws, X, Y, c.inner, steps, baseline, fault="left_endpoint").ig
    gap = completeness_gap(Ws, X, Y, c.inner, ig, baseline)
    gap.setflags(write=False)
    return gap


def model_gap(oracle_mod, case, baseline=0.0, steps=STEPS, rule="mid"):
    """the fp64 model's own gap per row on the fixture: the path rule's error, what no implementation can be asked to beat"""
    return _gap(oracle_mod, case.name, float(baseline), int(steps), rule)


LOSS_RTOL, LOSS_ATOL = 1e-4, 1e-5     # the suite's budget of one row's loss (tests/test_adversarial_gpu.py, test_pgd_gpu.py)


def delta_bound(oracle_mod, case, baseline, lx, lb):
    """per row: the model's worst recorded gap on the fixture + the row's element budgets summed + the loss budget of each of the
    two losses"""
    ref = reference(oracle_mod, case, baseline)
    worst = float(np.abs(model_gap(oracle_mod, case, baseline)).max())
    loss = (LOSS_RTOL * np.abs(lx) + LOSS_ATOL) + (LOSS_RTOL * np.abs(lb) + LOSS_ATOL)
    return worst + ref.budget.sum(axis=1) + loss
