"""The fp64 restatement of the input gradient (tests/input_gradient_cases.py) pinned on the CPU: against central differences of
both oracles' loss, at the kink, against a wrong kink rule, and -- for the fixtures the GPU test runs in bf16 -- the bf16 twin's
own scatter under another summation order (np_oracle._jittered)."""
import numpy as np
import pytest

from tests import input_gradient_cases as igc
from tests import np_oracle as npo

H = 1e-6            # central-difference step
FD_RTOL = 1e-6      # of max |g| (worst case seen over these shapes: 2e-7)
KINK_MARGIN = 0.05  # differenced coordinates are at least this far from the kink at 0


def _central(loss_fn, X, rows, cols):
    """d loss[row] / d X[row, col] by central differences, for every (row, col) pair of the two index arrays"""
    out = np.empty(len(rows))
    for k, (r, c) in enumerate(zip(rows, cols)):
        Xp, Xm = X.copy(), X.copy()
        Xp[r, c] += H
        Xm[r, c] -= H
        out[k] = (loss_fn(Xp)[r] - loss_fn(Xm)[r]) / (2 * H)
    return out


def _check_fd(oracle_mod, dims, X, Y, inner, out_kind, last, rows, cols):
    ref = oracle_mod.OracleNet(dims, out_kind=out_kind, inner_act=inner, last_act=last)
    Ws = npo.split(ref.get_weights(), dims)
    g = igc.input_gradient(Ws, X, Y, inner, out_kind, last)
    bound = FD_RTOL * np.abs(g).max()
    assert np.abs(g).max() > 0
    for name, loss_fn in (("np_oracle.loss", lambda x: npo.loss(Ws, x, Y, inner, out_kind, last)),
                          ("OracleNet.calculate_loss", lambda x: ref.calculate_loss(x, Y))):
        fd = _central(loss_fn, X, rows, cols)
        err = np.abs(fd - g[rows, cols]).max()
        print("%s: central differences off by %.3g (bound %.3g)" % (name, err, bound))
        assert err <= bound, (name, err, bound)


@pytest.mark.parametrize("out_kind", [igc.SCE, igc.GEN])
@pytest.mark.parametrize("inner", [igc.LEAKY, igc.SIGMOID, igc.TANH, igc.RELU, igc.IDENT])
def test_restatement_equals_central_differences(oracle_mod, inner, out_kind):
    dims, B = [12, 9, 7, 5], 4
    rng = np.random.default_rng(100 + 10 * inner + out_kind)
    X = KINK_MARGIN + (1 - KINK_MARGIN) * rng.random((B, dims[0]))
    Y = np.eye(dims[-1])[rng.integers(0, dims[-1], B)]
    rows, cols = np.divmod(np.arange(B * dims[0]), dims[0])
    _check_fd(oracle_mod, dims, X, Y, inner, out_kind, igc.SIGMOID, rows, cols)


@pytest.mark.parametrize("name", ["one_row", "two_layer", "ragged", "zeros", "general"])
def test_restatement_equals_central_differences_on_fixtures(oracle_mod, name):
    c = igc.BY_NAME[name]
    X, Y = igc.batch(c)
    rows, cols = np.nonzero(np.abs(X) >= KINK_MARGIN)
    pick = np.random.default_rng(c.seed).permutation(len(rows))[:40]
    _check_fd(oracle_mod, c.dims, X, Y, c.inner, c.out_kind, c.last, rows[pick], cols[pick])


@pytest.mark.parametrize("inner,at_zero", [(igc.LEAKY, 0.01), (igc.RELU, 0.0)])
def test_kink_rule_at_exact_zero(oracle_mod, inner, at_zero):
    """MT:235: `a <= 0 ? 0.01 : 1` -- an exact-zero input takes the left branch."""
    dims = [6, 5, 4]
    rng = np.random.default_rng(5)
    X = 0.1 + rng.random((3, dims[0]))
    X[:, ::2] = 0.0
    Y = np.eye(dims[-1])[[0, 3, 1]]
    Ws = npo.split(oracle_mod.OracleNet(dims, inner_act=inner).get_weights(), dims)
    g = igc.input_gradient(Ws, X, Y, inner)
    bare = igc.input_gradient(Ws, X, Y, inner, input_prime=lambda kind, z: np.ones_like(z))   # (delta_1 . W_0^T) alone
    assert np.abs(bare[:, ::2]).min() > 0
    assert np.array_equal(g[:, ::2], bare[:, ::2] * at_zero)
    assert np.array_equal(g[:, 1::2], bare[:, 1::2])


def test_wrong_kink_rule_is_far_outside_the_f32_budget(oracle_mod):
    """The GPU test's f32 budget tells `a <= 0` from `a < 0` on the exact-zero fixture: the two restatements lie more than a
    hundred budgets apart (about 0.8 max|g|, against 2e-3 max|g|)."""
    c = igc.BY_NAME["zeros"]
    X, Y = igc.batch(c)
    assert 0.1 < np.mean(X != 0) < 0.3
    right = igc.reference(oracle_mod, c)
    wrong = igc.input_gradient(igc.weights(oracle_mod, c), X, Y, c.inner, c.out_kind, c.last, input_prime=igc.wrong_rule_prime)
    off = np.abs(wrong - right).max() / np.abs(right).max()
    print("wrong rule: %.3g max|g| off" % off)
    assert off > 100 * igc.F32_RTOL


@pytest.mark.parametrize("name", [c.name for c in igc.BF16_CASES])
def test_bf16_fixtures_scatter_within_half_the_budget(oracle_mod, name):
    """A fixture is run in bf16 on the GPU only if the bf16 restatement itself, with every rounded operand moved by 1e-6
    relative before the rounding (another summation order), stays within half the bf16 budget over 8 draws."""
    c = igc.BY_NAME[name]
    X, Y = igc.batch(c)
    Ws = igc.weights(oracle_mod, c)
    ref = igc.reference(oracle_mod, c, bf16=True)
    scatter = max(np.abs(igc.input_gradient_bf16(Ws, X, Y, c.inner, c.out_kind, c.last, (1e-6, np.random.default_rng(k))) - ref).max()
                  for k in range(1, 9))
    rel = scatter / np.abs(ref).max()
    print("%s: scatter %.3g max|g|" % (name, rel))
    assert rel <= 0.5 * igc.BF16_RTOL


def test_headline_fixture_is_not_a_bf16_fixture():
    assert "headline" not in [c.name for c in igc.BF16_CASES]
    assert [c.name for c in igc.BF16_CASES] == ["ragged", "zeros", "baseline"]


def test_fgsm_direction_on_the_cpu(oracle_mod):
    """The GPU test's fgsm check with the restatement in the device's place: the same rows, the same 40 train_range steps from
    Random(1), the same eps -- the mean loss on clip(X + eps sign(g)) is above the mean loss on X."""
    c = igc.BY_NAME["zeros"]
    n, B, steps, step, momentum, eps = igc.FGSM
    X, Y = igc.make_rows(c.dims, n, c.seed + 400, c.density)
    w = np.array(oracle_mod.OracleNet(c.dims, inner_act=c.inner).get_weights())
    v = np.zeros_like(w)
    for s in range(steps):     # train_range: batch s of the data set, cyclically
        r0 = (s % (n // B)) * B
        w, v = npo.gradient_step(w, v, c.dims, X[r0:r0 + B], Y[r0:r0 + B], step, momentum, c.inner)
    Ws = npo.split(w, c.dims)
    adv = np.clip(X + eps * np.sign(igc.input_gradient(Ws, X, Y, c.inner)), 0.0, 1.0)
    before, after = npo.loss(Ws, X, Y, c.inner).mean(), npo.loss(Ws, adv, Y, c.inner).mean()
    print("mean loss %.4g -> %.4g" % (before, after))
    assert after > before
