"""What the fixtures of tests/adversarial_cases.py can show, from the fp64 model alone: few elements whose sign depends on who
computed the gradient, restatements in float32 and with bf16 operands that agree with the model on all the others, rows on
which the clip acts and pixels that stay zero, and six ways to get the kernel wrong that each move decided elements."""
import numpy as np
import pytest

from tests import adversarial_cases as ac
from tests import np_oracle as npo

ALL = [(c.name, False) for c in ac.CASES] + [(c.name, True) for c in ac.BF16_CASES]
FAULT_CLIP = (0.125, 0.875)   # lo > 0: a cell that should be an exact zero and goes through the formula becomes lo


def _fixture(oracle_mod, name, bf16, held=False):
    c = ac.BY_NAME[name]
    X, Y = ac.held_rows(c) if held else ac.rows(c)
    g = ac.reference_gradient(oracle_mod, c, bf16, held)
    return c, X, Y, g, ac.decided(g, X, c.inner, bf16)


@pytest.mark.parametrize("held", [False, True])
@pytest.mark.parametrize("name,bf16", ALL)
def test_undecided_share_is_below_the_cap(oracle_mod, name, bf16, held):
    c, X, Y, g, dec = _fixture(oracle_mod, name, bf16, held)
    share = 1.0 - dec.mean()
    print("%s %s%s: %d of %d elements undecided (%.3g %%), %d zero by structure" % (
        name, "bf16" if bf16 else "f32", " held-out" if held else "", (~dec).sum(), dec.size, 100 * share,
        (npo.act_prime(c.inner, X) == 0).sum()))
    assert np.abs(g).max() > 0
    assert share <= ac.UNDECIDED_CAP


@pytest.mark.parametrize("name", [c.name for c in ac.CASES])
def test_float32_restatement_agrees_on_decided_elements(oracle_mod, name):
    """the formulas carried in float32 stay inside the budget that defines `decided`, so their signs -- and the perturbed rows
    in float32 arithmetic -- are the model's there, for both eps"""
    c, X, Y, g, dec = _fixture(oracle_mod, name, False)
    g32 = ac.gradient_f32(ac.weights(oracle_mod, c), X, Y, c.inner)
    assert g32.dtype == np.float32
    assert np.abs(g32 - g).max() <= ac.budget(g)
    assert np.array_equal(ac.sign(g32)[dec], ac.sign(g)[dec])
    for eps in ac.EPS:
        want = ac.perturb(X, g, eps).astype(np.float32)
        got = ac.perturb(X, g32, eps, dtype=np.float32)
        assert got.dtype == np.float32
        assert np.array_equal(got[dec], want[dec])


@pytest.mark.parametrize("name", [c.name for c in ac.BF16_CASES])
def test_bf16_restatement_agrees_on_decided_elements(oracle_mod, name):
    """another summation order in front of the bf16 roundings (np_oracle._jittered) moves g by less than the bf16 budget"""
    c, X, Y, g, dec = _fixture(oracle_mod, name, True)
    for seed in range(3):
        gj = ac.gradient(ac.weights(oracle_mod, c), X, Y, c.inner, True, (1e-6, np.random.default_rng(seed)))
        assert np.abs(gj - g).max() <= ac.budget(g, True)
        assert np.array_equal(ac.sign(gj)[dec], ac.sign(g)[dec])
        assert np.array_equal(ac.perturb(X, gj, 0.1, dtype=np.float32)[dec], ac.perturb(X, g, 0.1).astype(np.float32)[dec])


@pytest.mark.parametrize("name,bf16", ALL)
def test_eps_zero_returns_the_rows(oracle_mod, name, bf16):
    c, X, Y, g, _ = _fixture(oracle_mod, name, bf16)
    got = ac.perturb(X, g, 0.0, dtype=np.float32)
    assert np.array_equal(got.view(np.uint32), X.astype(np.float32).view(np.uint32))


@pytest.mark.parametrize("name", [c.name for c in ac.CASES if c.n >= 16])
def test_the_clip_acts(oracle_mod, name):
    """decided elements on hi that the gradient pushes up and on lo that it pushes down: they stay where they are"""
    c, X, Y, g, dec = _fixture(oracle_mod, name, False)
    adv = ac.perturb(X, g, 0.1)
    up, down = dec & (X == 1.0) & (g > 0), dec & (X == 0.0) & (g < 0)
    assert up.sum() >= 3 and (down.sum() >= 1 or c.inner == ac.RELU), (up.sum(), down.sum())   # (a ReLU net's zero pixels have g == 0)
    assert np.all(adv[up] == 1.0) and np.all(adv[down] == 0.0)
    assert adv.min() >= 0.0 and adv.max() <= 1.0 and np.abs(adv - X).max() <= float(np.float32(0.1))
    moved = dec & (adv != X)
    assert moved.mean() > 0.1


def test_exact_zero_pixels_of_a_relu_net_stay_zero(oracle_mod):
    c, X, Y, g, dec = _fixture(oracle_mod, "relu_zeros", False)
    zero = X == 0.0
    assert zero.mean() > 0.4
    assert np.all(g[zero] == 0.0) and np.all(dec[zero])
    assert np.all(ac.perturb(X, g, 0.1)[zero] == 0.0)
    acc = ac.product(ac.weights(oracle_mod, c), X, Y, c.inner)
    assert np.all(acc[zero] != 0.0)     # (the product itself has a sign there: only f' makes the zero)


FAULT_FIXTURES = {
    "neighbour_row": [c.name for c in ac.CASES if c.n >= 2],
    "neighbour_quad": [c.name for c in ac.CASES],
    "no_fprime": ["relu_zeros"],
    "clip_first": [c.name for c in ac.CASES if c.n >= 16],
    "pad_columns": [c.name for c in ac.CASES if c.dims[0] % 16],
    "dead_rows": [c.name for c in ac.CASES if c.n % 16],
}


@pytest.mark.parametrize("fault,name", [(f, n) for f in ac.FAULTS for n in FAULT_FIXTURES[f]])
def test_a_fault_moves_cells_that_cannot_be_blurred(oracle_mod, fault, name):
    """The buffer a wrong kernel would write differs from the right one on decided live cells (more than a handful), or -- the
    two padding faults, with lo > 0 -- on cells that must be exact zeros: the padding columns are operands of the next forward
    and gradient products, the rows behind the block lie in the tiles those products read."""
    c, X, Y, g, dec = _fixture(oracle_mod, name, False)
    fp = npo.act_prime(c.inner, X)
    acc = ac.product(ac.weights(oracle_mod, c), X, Y, c.inner)
    assert np.array_equal(acc * fp, g)
    clip = FAULT_CLIP if fault in ("pad_columns", "dead_rows") else ac.CLIP
    right = ac.device_buffer(X, acc, fp, 0.1, clip)
    wrong = ac.device_buffer(X, acc, fp, 0.1, clip, fault)
    assert np.array_equal(right[:c.n, :c.dims[0]], ac.perturb(X, g, 0.1, clip))
    assert np.all(right[c.n:] == 0) and np.all(right[:, c.dims[0]:] == 0)
    if fault in ("pad_columns", "dead_rows"):
        pad = np.ones(right.shape, dtype=bool)
        pad[:c.n, :c.dims[0]] = False
        assert (wrong[pad] != 0).sum() >= 6 and np.all(wrong[pad][wrong[pad] != 0] == FAULT_CLIP[0])
        return
    differs = (wrong[:c.n, :c.dims[0]] != right[:c.n, :c.dims[0]]) & dec
    print("%s on %s: %d decided cells differ" % (fault, name, differs.sum()))
    assert differs.sum() >= 3


def test_the_oracle_run_meets_no_undecided_element(gnn, oracle_mod):
    """The 40-iteration run the GPU test holds to the oracle: along the fp64 trajectory every element of every batch lies at
    least ORACLE_MARGIN budgets from a sign change (the device's own trajectory error, W_ATOL per step, moves g by far less), the
    run moves the weights by thousands of budgets, the perturbation in float32 arithmetic ends inside a hundredth of the budget,
    and a perturbation DOWN the gradient ends hundreds of budgets away."""
    t = ac.ORACLE_RUN
    X, Y = ac.train_rows(t)
    w0 = ac.reference_net(oracle_mod, t.dims, t.inner, t.seed).get_weights()
    idx = ac.draws(gnn, t)
    assert sum(len(i) for i in idx) > t.n_rows      # the epoch sampler refills inside the run
    w, v, margin = ac.train_model(w0, t, X, Y, idx)
    bud = ac.W_ATOL * ac.TRAIN_ITERATIONS
    print("oracle run: least |g| %.3g budgets, weights moved %.3g budgets" % (margin, np.abs(w - w0).max() / bud))
    assert margin >= ac.ORACLE_MARGIN
    assert np.abs(w - w0).max() > 1000 * bud
    w32, v32, _ = ac.train_model(w0, t, X, Y, idx, dtype=np.float32)
    assert max(np.abs(w32 - w).max(), np.abs(v32 - v).max()) <= bud / 100
    ww, vw, _ = ac.train_model(w0, t, X, Y, idx, wrong_sign=True)
    assert np.abs(ww - w).max() > 100 * bud
    plain, _, _ = ac.train_model(w0, t, X, Y, idx, eps=0.0)
    assert np.abs(plain - w).max() > 100 * bud      # (and training on the rows themselves is as far away)
