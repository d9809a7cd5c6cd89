"""The projected-gradient calls (gnn_mlp_pgd_set_range, gnn_mlp_evaluate_pgd_set_range, gnn_mlp_train_sampled_pgd): the fp64
model, its float32 restatement, the random start in numpy uint32, the fault models and the fixtures of tests/test_pgd_cpu.py and
tests/test_pgd_gpu.py.  No tests here.

The current iterate is a, the origin x0 (the resident row), g the input gradient at a (tests/adversarial_cases.py: gradient).
One step, every operation in f32 and rounded on its own:

    s  = (g > 0) - (g < 0)
    v  = a + alpha * s
    w  = min(max(v, x0 - eps), x0 + eps)      the ball around the ORIGIN
    a' = min(max(w, lo), hi)                  the box last

An undecided sign at step t changes every gradient after it, so nothing here compares whole trajectories of two implementations:
the model takes ONE step from a given iterate (teacher forcing), and `trajectory` is the model's own sequence of iterates, each
rounded to float32 -- rows are float32 values throughout, as the device holds them.  Decided / undecided and the cap are
tests/adversarial_cases.py's, per step.

The fixtures, their weights (SCALE = 0.2 times the reference net's Random(1) draw) and rows are tests/adversarial_cases.py's."""
import collections
import functools

import numpy as np

from tests import adversarial_cases as ac
from tests import np_oracle as npo

EPS, ALPHA, T = 0.1, 0.04, 4      # 4 x 0.04 > 0.1: the projection acts
CLIP = ac.CLIP
FAULT_CLIP = (0.125, 0.875)       # lo > 0: a padding cell that goes through the formula becomes lo; rows outside the box
START_SEED = 7
# the fixtures whose bf16 trajectory keeps the undecided share under the cap at every step (the issue's table: one_row up to 10 %,
# blocks_dense up to 5.07 %; those two run in the bitwise twin checks alone)
BF16_MODEL_CASES = [c for c in ac.BF16_CASES if c.name in ("ident", "relu_zeros")]
MODEL_CASES = [(c.name, False) for c in ac.CASES] + [(c.name, True) for c in BF16_MODEL_CASES]


def f32(x):
    return np.float32(x)


# ---- the step ---------------------------------------------------------------------------------------------------------------------
def step(a, x0, g, eps=EPS, alpha=ALPHA, clip=CLIP, dtype=np.float64, s=None):
    """One step in `dtype` (np.float32: the device's arithmetic).  eps, alpha and the bounds are the float32 values the call is
    defined with; on float32 rows every fp64 sum below is exact, so the fp64 result rounded to float32 is the float32 result.
    s: a sign array to use instead of sign(g)."""
    a, x0 = np.asarray(a, dtype=dtype), np.asarray(x0, dtype=dtype)
    s = (ac.sign(np.asarray(g)) if s is None else np.asarray(s)).astype(dtype)
    e, al, lo, hi = dtype(f32(eps)), dtype(f32(alpha)), dtype(f32(clip[0])), dtype(f32(clip[1]))
    v = a + al * s
    w = np.minimum(np.maximum(v, x0 - e), x0 + e)
    return np.minimum(np.maximum(w, lo), hi)


def feasible(x0, eps=EPS, clip=CLIP):
    """[max(lo, x0 - eps), min(hi, x0 + eps)] as f32 forms them: where every element of every iterate lies"""
    x0 = np.asarray(x0, dtype=np.float32)
    return np.maximum(f32(clip[0]), x0 - f32(eps)), np.minimum(f32(clip[1]), x0 + f32(eps))


# ---- the random start ------------------------------------------------------------------------------------------------------------
def mix(u):
    u = np.asarray(u, dtype=np.uint32)
    u = u ^ (u >> np.uint32(16))
    u = u * np.uint32(0x7feb352d)
    u = u ^ (u >> np.uint32(15))
    u = u * np.uint32(0x846ca68b)
    return u ^ (u >> np.uint32(16))


def start_u(seed, rows, d0, n=0):
    """u in [-1, 1), float32, exact: rows x d0.  rows: the rows' indices in their resident set."""
    rows = np.asarray(rows, dtype=np.int64).astype(np.uint32)
    with np.errstate(over="ignore"):
        r = mix(mix(mix(np.array([seed], dtype=np.uint32)) + np.uint32(n)) ^ rows)
        h = mix(r[:, None] + np.uint32(0x9E3779B9) * np.arange(d0, dtype=np.uint32)[None, :])
    return (h >> np.uint32(8)).astype(np.float32) * f32(2.0 ** -23) - f32(1.0)


def start(X, seed, rows, eps=EPS, clip=CLIP, n=0):
    """a_0 = min(max(x0 + eps * u, lo), hi) in float32: two roundings, then the box"""
    x0 = np.asarray(X, dtype=np.float32)
    v = x0 + f32(eps) * start_u(seed, rows, x0.shape[1], n)
    return np.minimum(np.maximum(v, f32(clip[0])), f32(clip[1]))


# ---- the model's own trajectory on a fixture ---------------------------------------------------------------------------------------
Trajectory = collections.namedtuple("Trajectory", "xs gs")     # xs[t]: the iterate after t steps (fp64 of float32); gs[t]: g at xs[t]


def run(Ws, X, Y, inner, bf16=False, steps=T, eps=EPS, alpha=ALPHA, clip=CLIP, a0=None):
    xs, gs = [np.asarray(X if a0 is None else a0, dtype=np.float64)], []
    for _ in range(steps):
        g = ac.gradient(Ws, xs[-1], Y, inner, bf16)
        gs.append(g)
        xs.append(step(xs[-1], X, g, eps, alpha, clip).astype(np.float32).astype(np.float64))
    return Trajectory(xs, gs)


@functools.lru_cache(maxsize=None)
def _trajectory(oracle_mod, name, bf16):
    c = ac.BY_NAME[name]
    X, Y = ac.rows(c)
    tr = run(ac.weights(oracle_mod, c), X, Y, c.inner, bf16)
    for a in tr.xs + tr.gs:
        a.setflags(write=False)
    return tr


def trajectory(oracle_mod, case, bf16=False):
    """the model's T steps on the fixture's rows, no random start, computed once and shared (read-only)"""
    return _trajectory(oracle_mod, case.name, bool(bf16))


# ---- the fault models: what a wrong kernel would store ---------------------------------------------------------------------------
def step_buffer(a, x0, g, eps=EPS, alpha=ALPHA, clip=CLIP, fault=None):
    """The pad(B) x pad(d_0) rows buffer pgd_kernel writes for one step: live cells the formula, everything else exact zeros."""
    B, d0 = a.shape
    Bp, dp = ac.pad16(B), ac.pad16(d0)
    A, X0, G = ac.padded(np.asarray(a, dtype=np.float64), Bp, dp), ac.padded(np.asarray(x0, dtype=np.float64), Bp, dp), ac.padded(g, Bp, dp)
    e, al, lo, hi = float(f32(eps)), float(f32(alpha)), float(f32(clip[0])), float(f32(clip[1]))
    if fault == "ball_iterate":         # the ball taken around the current iterate, not the origin
        out = step(A, A, G, eps, alpha, clip)
    elif fault == "box_first":          # the box before the ball
        v = np.minimum(np.maximum(A + al * ac.sign(G), lo), hi)
        out = np.minimum(np.maximum(v, X0 - e), X0 + e)
    elif fault == "alpha_eps":          # alpha and eps exchanged
        out = step(A, X0, G, alpha, eps, clip)
    else:
        out = step(A, X0, G, eps, alpha, clip)
    r, c = np.arange(Bp)[:, None], np.arange(dp)[None, :]
    live = (r < B) & (c < d0)
    if fault == "pad_columns":
        live = np.broadcast_to(r < B, live.shape)
    elif fault == "dead_rows":
        live = np.broadcast_to(c < d0, live.shape)
    return np.where(live, out, 0.0)


STEP_FAULTS = ("ball_iterate", "box_first", "alpha_eps", "pad_columns", "dead_rows")


def start_buffer(X, seed, first, max_batch, eps=EPS, clip=CLIP, n=0, fault=None):
    """The start rows of a range [first, first + len(X)) taken in blocks of max_batch, as pgd_start_kernel writes them (live cells
    only).  X: the range's rows."""
    X = np.asarray(X, dtype=np.float32)
    out = np.empty_like(X)
    for off in range(0, len(X), max_batch):
        B = min(max_batch, len(X) - off)
        rows = np.arange(B) + (0 if fault == "block_local_row" else first + off)   # keyed by the block-local row
        out[off:off + B] = start(X[off:off + B], seed, rows, eps, clip, 0 if fault == "ignores_n" else n)
    return out


# ---- adversarial training: the model of gnn_mlp_train_sampled_pgd -------------------------------------------------------------------
TRAIN_T = 3
TRAIN_ITERATIONS = ac.TRAIN_ITERATIONS    # the exact-twin runs (ac.TWIN_RUNS): 40 iterations, the epoch sampler refills
TRAIN_ALPHA = 0.04
# The oracle run is tests/adversarial_cases.py's ORACLE_RUN (8-6-4, batch 8 on 300 rows) with TRAIN_T steps and no random start,
# SHORTENED to 27 iterations: over 40 x 3 gradient evaluations the least |g| is 8.6 budgets (met in iteration 28), under the
# margin of 10 the run has to hold; over the first 27 x 3 it is 16.2 budgets.  27 is the longest run that holds the margin, and
# tests/test_pgd_cpu.py holds it there.  (27 x 8 draws do not exhaust the 300 rows: the refill is the twin runs' to cover.)
ORACLE_RUN = ac.ORACLE_RUN
ORACLE_ITERATIONS = 27


def train_model(w0, t, X, Y, idx_lists, steps=TRAIN_T, eps=ac.TRAIN_EPS, alpha=TRAIN_ALPHA, clip=CLIP, origin_fault=False,
                dtype=np.float64):
    """fp64: per iteration the batch attacked against the weights of that moment (iterates rounded to float32 after every step, as
    the device holds them), then gradientStep (SCE:297-346) on the result.  Returns (w, v, least |g| / budget over every element
    of every gradient evaluation).  origin_fault: the origin of row b taken as dataset row b, not idx[b].  dtype=np.float32: the
    step (alone) in the device's arithmetic."""
    step_size, momentum = ac.TRAIN_HYPER
    w, v = np.array(w0, dtype=np.float64), np.zeros(len(w0))
    margin = np.inf
    for idx in idx_lists:
        Xb, Yb = X[idx], Y[idx]
        x0 = X[:len(idx)] if origin_fault else Xb
        a = Xb
        for _ in range(steps):
            g = ac.gradient(npo.split(w, t.dims), a, Yb, t.inner)
            margin = min(margin, float(np.abs(g).min()) / ac.budget(g))
            a = step(a, x0, g, eps, alpha, clip, dtype).astype(np.float32).astype(np.float64)
        w, v = npo.gradient_step(w, v, t.dims, a, Yb, step_size, momentum, t.inner)
    return w, v, margin
