"""Input gradients (gnn_mlp_input_gradient*): the fp64 restatement and the seeded fixtures of tests/test_input_gradient_cpu.py
and tests/test_input_gradient_gpu.py.  No tests here.

The restatement continues np_oracle.gradient's backward loop to l = 0, with np_oracle's own pieces:

    D = (D @ Ws[0].T) * act_prime(inner, Z[0])            g = d calculateLoss(x, y) / d x, one row per input row

(f' appears because the reference applies f to the raw input too, SCE:183-186).  The bf16 twin takes delta_1 and W_0 rounded to
bf16 -- (q(D) @ q(Ws[0]).T) * act_prime(inner, Z[0]) -- on np_oracle._forward_bf16 and gradient_bf16's loop, with _jittered."""
import collections
import functools

import numpy as np

from tests import np_oracle as npo

LEAKY, SIGMOID, TANH, RELU, IDENT = range(5)
SCE, GEN = 0, 1

Case = collections.namedtuple("Case", "name dims B inner out_kind last seed density bf16")

# the smallest shapes at which the kernel can still go wrong (what each pins: the issue's table)
CASES = [
    Case("one_row", [5, 4, 3, 3], 1, LEAKY, SCE, SIGMOID, 11, 1.0, False),        # one row; everything inside one padded tile
    Case("two_layer", [64, 10], 7, RELU, SCE, SIGMOID, 12, 0.5, False),           # delta_1 is the output delta; exact-zero inputs
    Case("ragged", [20, 17, 33, 7], 19, TANH, SCE, SIGMOID, 13, 1.0, True),       # d_0 -> 32, d_1 17 -> 32 (two k chunks), B -> 32
    Case("zeros", [100, 40, 24, 10], 17, LEAKY, SCE, SIGMOID, 14, 0.19, True),    # the `a <= 0` rule at exact zeros
    Case("baseline", [784, 100, 50, 10], 32, SIGMOID, SCE, SIGMOID, 15, 1.0, True),  # a BASELINE shape on the two-launch path
    Case("headline", [784, 300, 100, 10], 128, LEAKY, SCE, SIGMOID, 16, 0.19, False),  # f32 only (its bf16 scatter: 3.9e-3)
    Case("general", [20, 17, 33, 7], 19, SIGMOID, GEN, SIGMOID, 17, 1.0, False),  # GNN:267-271 output delta
    Case("gemm_plan", [1025, 374, 30], 16, LEAKY, SCE, SIGMOID, 18, 1.0, False),  # a net the two-launch plan refuses
]
BY_NAME = {c.name: c for c in CASES}
BF16_CASES = [c for c in CASES if c.bf16]

F32_RTOL, F32_ATOL = 2e-5, 1e-9     # test_parity_gpu.py's budget for weight gradients
BF16_RTOL, BF16_ATOL = 4e-3, 1e-7   # test_bf16_gpu.py's budget

# the fgsm direction check on the "zeros" net: rows, batch, train_range steps, step size, momentum, eps
FGSM = (64, 16, 40, 0.05, 0.9, 0.1)


def make_rows(dims, n, seed, density=1.0):
    """n seeded rows: X ~ U[0, 1) thinned to `density` non-zeros (exact zeros elsewhere), Y one-hot."""
    rng = np.random.default_rng(seed)
    X = rng.random((n, dims[0]))
    if density < 1.0:
        X *= rng.random((n, dims[0])) < density
    Y = np.eye(dims[-1])[rng.integers(0, dims[-1], n)]
    return X, Y


def batch(case):
    return make_rows(case.dims, case.B, case.seed, case.density)


def _output_delta(Z, out, Y, out_kind, last):
    return out - Y if out_kind == 0 else (out - Y) * npo.act_prime(last, Z[-1])   # SCE:249-251 / GNN:267-271


def input_gradient(Ws, X, Y, inner, out_kind=0, last=1, input_prime=npo.act_prime):
    """fp64; input_prime: the f' of the l = 0 factor (a test swaps in a wrong rule)."""
    Z, out = npo.forward(Ws, X, inner, out_kind, last)
    D = _output_delta(Z, out, Y, out_kind, last)
    for l in range(len(Ws) - 1, 0, -1):
        D = (D @ Ws[l].T) * npo.act_prime(inner, Z[l])      # SCE:272-278
    return (D @ Ws[0].T) * input_prime(inner, Z[0])


def input_gradient_bf16(Ws, X, Y, inner, out_kind=0, last=1, jitter=None):
    q = npo.bf16_round
    Z, _, _, out = npo._forward_bf16(Ws, X, inner, out_kind, last, jitter)
    D = _output_delta(Z, out, Y, out_kind, last)
    for l in range(len(Ws) - 1, 0, -1):
        D = (q(npo._jittered(D, jitter)) @ q(Ws[l]).T) * npo.act_prime(inner, Z[l])
    return (q(npo._jittered(D, jitter)) @ q(Ws[0]).T) * npo.act_prime(inner, Z[0])


def wrong_rule_prime(kind, z):
    """`a < 0` where MT:235 says `a <= 0`: differs at exact zeros only."""
    if kind == LEAKY:
        return np.where(z < 0, 0.01, 1.0)
    if kind == RELU:
        return np.where(z < 0, 0.0, 1.0)
    return npo.act_prime(kind, z)


def reference_net(oracle_mod, case, seed=1):
    return oracle_mod.OracleNet(case.dims, out_kind=case.out_kind, inner_act=case.inner, last_act=case.last, seed=seed)


@functools.lru_cache(maxsize=None)
def _weights(oracle_mod, name, seed):
    c = BY_NAME[name]
    w = reference_net(oracle_mod, c, seed).get_weights()
    w.setflags(write=False)
    return w


def weights(oracle_mod, case, seed=1):
    """the reference net's Random(seed) weights (SCE:139-156), as the list of layer matrices"""
    return npo.split(_weights(oracle_mod, case.name, seed), case.dims)


@functools.lru_cache(maxsize=None)
def _reference(oracle_mod, name, bf16):
    c = BY_NAME[name]
    X, Y = batch(c)
    fn = input_gradient_bf16 if bf16 else input_gradient
    g = fn(weights(oracle_mod, c), X, Y, c.inner, c.out_kind, c.last)
    g.setflags(write=False)
    return g


def reference(oracle_mod, case, bf16=False):
    """the restatement on the fixture's batch, computed once and shared (read-only)"""
    return _reference(oracle_mod, case.name, bool(bf16))


def within(g, ref, bf16=False):
    """(worst |g - ref|, the budget) over the call"""
    rtol, atol = (BF16_RTOL, BF16_ATOL) if bf16 else (F32_RTOL, F32_ATOL)
    return float(np.abs(g - ref).max()), rtol * float(np.abs(ref).max()) + atol
