"""The fast-gradient-sign calls (gnn_mlp_fgsm_set_range, gnn_mlp_evaluate_fgsm_set_range, gnn_mlp_train_sampled_fgsm): the fp64
model and the seeded fixtures of tests/test_adversarial_cpu.py and tests/test_adversarial_gpu.py.  No tests here.

The model is tests/input_gradient_cases.py's restatement of the input gradient g with the perturbation behind it:

    x' = min(max(x + eps * s(g), lo), hi),   s(g) = (g > 0) - (g < 0)

An element is DECIDED when its sign cannot depend on who computed g: |g| above the suite's input-gradient budget (2e-5 max|g| f32,
4e-3 max|g| bf16, + the budgets' absolute terms), or g exactly zero BY STRUCTURE -- f'(a0) = 0, a ReLU net's exact-zero pixel,
where every implementation multiplies by an exact 0.  The other elements are UNDECIDED; tests/test_adversarial_cpu.py holds
their share below 5 % of the live elements in every fixture.

Rows are drawn in float32 (stored as fp64): the device's f32 copy of an uploaded row is then the row itself."""
import collections
import functools

import numpy as np

from tests import input_gradient_cases as igc
from tests import np_oracle as npo

LEAKY, SIGMOID, TANH, RELU, IDENT = range(5)

Case = collections.namedtuple("Case", "name dims n max_batch inner seed density bf16")

# the smallest shapes at which the kernel's geometry can go wrong: d_0 no multiple of 64 or of 16 (70, 200, 784), d_1 no multiple
# of 16 (30, 100, 10), B in {1, 17, 37}, ranges of 2 max_batch + 5 rows, the three activations, the plans beside the two-launch one
CASES = [
    Case("one_row", [70, 30, 10], 1, 1, LEAKY, 31, 1.0, True),                # one row: 15 dead rows in its tile
    Case("relu_zeros", [200, 30, 24, 10], 17, 17, RELU, 32, 0.5, True),       # exact-zero pixels: g == 0 there, the pixel stays 0
    Case("ident", [70, 30, 10], 37, 37, IDENT, 33, 1.0, True),                # three row tiles, the last with 5 live rows
    Case("blocks", [784, 100, 50, 10], 69, 32, LEAKY, 34, 0.19, False),       # two-launch plan; two blocks and a ragged one
    Case("blocks_dense", [784, 100, 50, 10], 69, 32, LEAKY, 35, 1.0, True),   # ... in bf16 too (a leaky net's zero pixels have
                                                                              # |g| a hundredth of the others': undecided in bf16)
    Case("per_layer", [70, 10], 17, 17, LEAKY, 36, 1.0, False),               # per-layer GEMMs; delta_1 is the output delta
    Case("gemm_plan", [1025, 374, 30], 16, 16, LEAKY, 37, 1.0, False),        # a net the two-launch plan refuses (three launches)
    Case("hybrid", [200, 512, 272, 10], 27, 27, LEAKY, 38, 0.19, False),      # middle weights beyond LDS: the hybrid plan
]
BY_NAME = {c.name: c for c in CASES}
BF16_CASES = [c for c in CASES if c.bf16]

EPS = (0.0, 0.1)
CLIP = (0.0, 1.0)
UNDECIDED_CAP = 0.05
# The reference draws weights from U(-0.5, 0.5) (SCE:139-156): at these widths the softmax saturates, most rows carry a gradient
# thousands of times below the largest and a fifth of the elements would be undecided.  Every fixture net therefore starts from
# SCALE times its Random(seed) weights (set_weights on the device): the undecided shares are then 0.6 % (f32) and 4.3 % (bf16) at most.
SCALE = 0.2
ON_HI, ON_LO = 0.05, 0.01   # shares of the elements put exactly on hi / (dense fixtures) on lo, so that the clip acts


def make_rows(dims, n, seed, density=1.0):
    """n seeded rows, exact in float32: U[0, 1) thinned to `density` non-zeros, ON_HI of the elements exactly 1, ON_LO exactly 0;
    Y one-hot."""
    rng = np.random.default_rng(seed)
    X = rng.random((n, dims[0])).astype(np.float32)
    if density < 1.0:
        X *= rng.random((n, dims[0])) < density
    X[rng.random((n, dims[0])) < ON_HI] = 1.0
    X[rng.random((n, dims[0])) < ON_LO] = 0.0
    Y = np.eye(dims[-1])[rng.integers(0, dims[-1], n)]
    return X.astype(np.float64), Y


def rows(case):
    return make_rows(case.dims, case.n, case.seed, case.density)


def held_rows(case):
    """a second set of the same kind, for the held-out calls"""
    return make_rows(case.dims, case.n, case.seed + 500, case.density)


def sign(g):
    return (g > 0).astype(g.dtype) - (g < 0).astype(g.dtype)


def perturb(a0, g, eps, clip=CLIP, dtype=np.float64):
    """The formula, every operation in `dtype` (np.float32: the device's arithmetic, one rounding per operation).  eps and the
    bounds are the float32 values the call is defined with: on float32 rows the fp64 sum a0 + eps * s is then exact, and its
    rounding to float32 is the float32 sum."""
    a0, s = np.asarray(a0, dtype=dtype), sign(np.asarray(g)).astype(dtype)
    clip = (np.float32(clip[0]), np.float32(clip[1]))
    t = dtype(np.float32(eps)) * s
    v = a0 + t
    return np.minimum(np.maximum(v, dtype(clip[0])), dtype(clip[1]))


def gradient(Ws, X, Y, inner, bf16=False, jitter=None):
    """fp64 input gradient of the softmax / cross-entropy net; bf16: with the GEMM operands rounded (igc.input_gradient_bf16)"""
    if bf16:
        return igc.input_gradient_bf16(Ws, X, Y, inner, 0, 1, jitter)
    return igc.input_gradient(Ws, X, Y, inner)


def gradient_f32(Ws, X, Y, inner):
    """the same formulas carried in float32 (np_oracle.forward's dtype form): what an f32 device computes, in another order"""
    W32 = [W.astype(np.float32) for W in Ws]
    Z, out = npo.forward(W32, X, inner, 0, 1, np.float32)
    D = out - Y.astype(np.float32)
    for l in range(len(W32) - 1, 0, -1):
        D = (D @ W32[l].T) * npo.act_prime(inner, Z[l])
    return (D @ W32[0].T) * npo.act_prime(inner, Z[0])


def budget(g, bf16=False):
    rtol, atol = (igc.BF16_RTOL, igc.BF16_ATOL) if bf16 else (igc.F32_RTOL, igc.F32_ATOL)
    return rtol * float(np.abs(g).max()) + atol


def decided(g, a0, inner, bf16=False):
    """boolean mask: |g| above the budget of the call, or zero by structure (f'(a0) == 0)"""
    structural = npo.act_prime(inner, np.asarray(a0, dtype=np.float64)) == 0
    return (np.abs(g) > budget(g, bf16)) | structural


def reference_net(oracle_mod, dims, inner, seed=1):
    return oracle_mod.OracleNet(dims, out_kind=0, inner_act=inner, last_act=1, seed=seed)


@functools.lru_cache(maxsize=None)
def _weights(oracle_mod, dims, inner, seed):
    w = reference_net(oracle_mod, list(dims), inner, seed).get_weights()
    w.setflags(write=False)
    return w


def flat_weights(oracle_mod, case, seed=1):
    """SCALE times the reference net's Random(seed) weights (SCE:139-156), flat: what the fixture's device net is given"""
    w = SCALE * _weights(oracle_mod, tuple(case.dims), case.inner, seed)
    w.setflags(write=False)
    return w


def weights(oracle_mod, case, seed=1):
    """... as layer matrices"""
    return npo.split(flat_weights(oracle_mod, case, seed), case.dims)


@functools.lru_cache(maxsize=None)
def _reference(oracle_mod, name, bf16, held):
    c = BY_NAME[name]
    X, Y = held_rows(c) if held else rows(c)
    g = gradient(weights(oracle_mod, c), X, Y, c.inner, bf16)
    g.setflags(write=False)
    return g


def reference_gradient(oracle_mod, case, bf16=False, held=False):
    """the model's g on the fixture's rows, computed once and shared (read-only)"""
    return _reference(oracle_mod, case.name, bool(bf16), bool(held))


# ---- the fault models: what a wrong kernel would store (tests/test_adversarial_cpu.py shows that each moves decided elements) ----
def padded(a, rows_pad, cols_pad):
    out = np.zeros((rows_pad, cols_pad), dtype=a.dtype)
    out[:a.shape[0], :a.shape[1]] = a
    return out


def pad16(n):
    return (n + 15) // 16 * 16


def product(Ws, X, Y, inner):
    """acc = delta_1 . W_0^T, the input gradient before its factor f'(a0)"""
    return igc.input_gradient(Ws, X, Y, inner, input_prime=lambda kind, z: np.ones_like(z))


def device_buffer(a0, acc, fprime, eps, clip, fault=None):
    """The pad(B) x pad(d_0) rows buffer the kernel writes, from the product acc = delta_1 . W_0^T (g = acc * f'): live cells the
    formula, everything else exact zeros.  `fault` names one way to get it wrong."""
    B, d0 = a0.shape
    Bp, dp = pad16(B), pad16(d0)
    A, ACC, FP = padded(a0, Bp, dp), padded(acc, Bp, dp), padded(fprime, Bp, dp)
    G = ACC * FP
    r, c = np.arange(Bp)[:, None], np.arange(dp)[None, :]
    if fault == "neighbour_row":        # the sign of row b ^ 1 of the 16-row tile
        G = G[np.arange(Bp) ^ 1]
    elif fault == "neighbour_quad":     # the sign of the neighbouring quad of four columns
        G = G[:, ((np.arange(dp) // 4) ^ 1) * 4 + np.arange(dp) % 4]
    elif fault == "no_fprime":          # f' left out of the sign
        G = ACC
    if fault == "clip_first":           # the clip applied before the add
        out = np.minimum(np.maximum(A, clip[0]), clip[1]) + eps * sign(G)
    else:
        out = perturb(A, G, eps, clip)
    live = (r < B) & (c < d0)
    if fault == "pad_columns":          # the padding columns go through the formula too
        live = np.broadcast_to(r < B, live.shape)
    elif fault == "dead_rows":          # ... or the rows behind the block
        live = np.broadcast_to(c < d0, live.shape)
    return np.where(live, out, 0.0)


FAULTS = ("neighbour_row", "neighbour_quad", "no_fprime", "clip_first", "pad_columns", "dead_rows")


# ---- adversarial training: the model of gnn_mlp_train_sampled_fgsm -------------------------------------------------------------------
Train = collections.namedtuple("Train", "name dims inner n_rows batch seed data_seed")
TRAIN_ITERATIONS = 40
TRAIN_HYPER = (0.0125, 0.9)      # step size, momentum (the suite's trajectory budgets are stated for steps of this size)
TRAIN_EPS = 0.1
SAMPLER_SEED = 5
# exact-twin runs: batch 8 on 300 rows (40 x 8 = 320 draws: the epoch sampler refills), batch 37
TWIN_RUNS = [
    Train("two_launch_8", [100, 40, 24, 10], LEAKY, 300, 8, 1, 41),
    Train("two_launch_37", [100, 40, 24, 10], LEAKY, 300, 37, 1, 41),
    Train("per_layer_8", [70, 10], LEAKY, 300, 8, 1, 42),
    Train("per_layer_37", [70, 10], LEAKY, 300, 37, 1, 42),
]
# the oracle run: a net small enough that over 40 iterations NO element of any batch comes near a sign change (chosen by
# tests/test_adversarial_cpu.py::test_the_oracle_run_meets_no_undecided_element, which holds the margin)
ORACLE_RUN = Train("oracle", [8, 6, 4], LEAKY, 300, 8, 1, 12)
ORACLE_MARGIN = 10.0             # least |g| along the trajectory, in budgets of its batch
W_ATOL = 2e-6                    # per step, weights and momentum, f32 against fp64 (tests/test_trainer_gpu.py, test_chain_shapes_gpu.py)


def train_rows(t):
    """dense rows away from the kink (a leaky net's zero pixels carry a hundredth of the gradient), exact in float32"""
    rng = np.random.default_rng(1000 + t.data_seed)
    X = (0.05 + 0.9 * rng.random((t.n_rows, t.dims[0]))).astype(np.float32).astype(np.float64)
    Y = np.eye(t.dims[-1])[rng.integers(0, t.dims[-1], t.n_rows)]
    return X, Y


def draws(gnn, t, iterations=TRAIN_ITERATIONS):
    """the index vectors the epoch sampler (NNT:143-168) hands out, one per iteration"""
    s = gnn.Sampler(t.n_rows, seed=SAMPLER_SEED)
    out = [s.sample(t.batch) for _ in range(iterations)]
    s.close()
    return out


def train_model(w0, t, X, Y, idx_lists, eps=TRAIN_EPS, clip=CLIP, wrong_sign=False, dtype=np.float64):
    """fp64: per iteration the batch perturbed against the weights of that moment, then gradientStep (SCE:297-346) on the
    perturbed rows.  Returns (w, v, least |g| / budget over every element met).  wrong_sign: the perturbation DOWN the gradient;
    dtype=np.float32: the perturbation (alone) in the device's arithmetic."""
    step, momentum = TRAIN_HYPER
    w, v = np.array(w0, dtype=np.float64), np.zeros(len(w0))
    margin = np.inf
    for idx in idx_lists:
        Xb, Yb = X[idx], Y[idx]
        g = gradient(npo.split(w, t.dims), Xb, Yb, t.inner)
        margin = min(margin, float(np.abs(g).min()) / budget(g))
        Xa = perturb(Xb, -g if wrong_sign else g, eps, clip, dtype).astype(np.float64)
        w, v = npo.gradient_step(w, v, t.dims, Xa, Yb, step, momentum, t.inner)
    return w, v, margin
