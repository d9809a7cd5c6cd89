"""What the fixtures of tests/intgrad_cases.py can show, from the oracles alone: a float32 restatement well inside the element
budget, six ways to get the device route wrong that each leave it, the completeness gap of the fp64 model -- the path rule's own
error, which the device test's bound is built from -- and what more path points buy.

Figures of the fp64 model (worst row, steps = 8 -> 32; `left`: the left-endpoint rule at 8 points).  Baseline 0 and the identity
net have no kink on the path -- with b = 0 every pre-activation of a positively homogeneous net (leaky ReLU, ReLU, identity) is
alpha times its value at the row, so no unit changes side -- and there the gap falls sixteenfold from 8 to 32 points (1 / m^2)
and the left-endpoint rule is 900 to 320 000 times worse.  Baseline 0.25 moves hidden units of the leaky / ReLU nets across
their kink; the midpoint rule is then first-order like the left-endpoint one (gap 8 -> 32 falls 4 to 6 times, left / mid 1.1 to 5).

    fixture        b = 0: gap 8   gap 32    left      b = 0.25: gap 8   gap 32    left
    one_row        2.9e-7         1.8e-8    1.4e-2    1.9e-4            3.6e-5    1.0e-3
    relu_zeros     1.3e-8         7.9e-10   4.1e-3    1.2e-3            2.5e-4    2.6e-3
    ident          3.2e-7         2.0e-8    6.1e-4    2.5e-7            1.5e-8    3.8e-4
    blocks         6.5e-7         4.1e-8    2.5e-2    9.7e-3            2.5e-3    1.3e-2
    blocks_dense   1.5e-6         9.1e-8    3.0e-2    4.1e-3            1.1e-3    9.8e-3
    per_layer      3.2e-5         2.0e-6    1.2e-1    8.5e-6            5.3e-7    4.3e-3
    gemm_plan      3.6e-4         2.3e-5    3.9e-1    2.3e-2            4.0e-3    7.4e-2
    hybrid         2.0e-6         1.3e-7    4.2e-2    2.3e-2            5.3e-3    2.5e-2

(per_layer has no hidden layer: its path has no kink at either baseline.)"""
import numpy as np
import pytest

from tests import adversarial_cases as ac
from tests import intgrad_cases as ic

F32 = [c.name for c in ic.CASES]
# a fault is VISIBLE on a cell when it leaves four element budgets; the share it must reach is stated against the cells that can
# move at all: d != 0 (IG is d times a mean -- a zero pixel at baseline 0 has IG = 0 whatever the mean is)
VISIBLE = 4.0
SHARE = 0.75


def kink_free(c, baseline):
    """no unit changes side along the path: b = 0 (positive homogeneity), no inner nonlinearity, or no hidden layer"""
    return baseline == 0.0 or c.inner == ac.IDENT or len(c.dims) == 2


@pytest.mark.parametrize("baseline", ic.BASELINES)
@pytest.mark.parametrize("name,bf16", ic.ALL)
def test_float32_restatement_stays_inside_a_quarter_of_the_budget(oracle_mod, name, bf16, baseline):
    c = ac.BY_NAME[name]
    X, Y = ac.rows(c)
    ref = ic.reference(oracle_mod, c, baseline, bf16)
    got = ic.restatement(ac.weights(oracle_mod, c), X, Y, c.inner, ic.STEPS, baseline, bf16)
    err = np.abs(got.astype(np.float64) - ref.ig)
    worst = float((err / np.where(ref.budget > 0, ref.budget, 1.0)).max())
    print("%s %s b=%.2f: worst |restatement - model| %.3g budgets, max|IG| %.3g" % (name, "bf16" if bf16 else "f32", baseline, worst, np.abs(ref.ig).max()))
    assert np.abs(ref.ig).max() > 1e-3
    assert np.all(err <= 0.25 * ref.budget)
    assert np.all(ref.ig[ref.budget == 0] == 0)            # (d == 0: an exact zero either way)
    if baseline > 0:
        assert (np.asarray(ref.d) < 0).mean() > 0.2        # d is negative on many cells
    for a in ic.points(X, baseline, ic.STEPS)[1]:          # every point is a valid f(x): not negative
        assert np.all(a >= 0)


def test_one_step_is_the_midpoint_alone(oracle_mod):
    name, steps, baseline = ic.ONE_STEP
    c = ac.BY_NAME[name]
    X, Y = ac.rows(c)
    ref = ic.reference(oracle_mod, c, baseline, False, steps)
    assert len(ref.gs) == 1 and ic.alphas(1) == [np.float32(0.5)]
    got = ic.restatement(ac.weights(oracle_mod, c), X, Y, c.inner, steps, baseline)
    assert np.all(np.abs(got - ref.ig) <= 0.25 * ref.budget)
    assert np.array_equal(ref.ig, np.asarray(ref.d, dtype=np.float64) * ref.gs[0])


# (a stale sum needs a previous block: the fixtures of more than one block)
FAULT_RUNS = [(c.name, b, f) for c in ic.CASES for b in ic.BASELINES for f in ic.FAULTS
              if f != "no_fprime" and (f != "stale_sum" or c.n > c.max_batch)]


@pytest.mark.parametrize("name,baseline,fault", FAULT_RUNS)
def test_each_fault_leaves_the_budget(oracle_mod, name, baseline, fault):
    c = ac.BY_NAME[name]
    X, Y = ac.rows(c)
    ref = ic.reference(oracle_mod, c, baseline)
    bad = ic.model(ac.weights(oracle_mod, c), X, Y, c.inner, ic.STEPS, baseline, False, fault, c.max_batch).ig
    out = np.abs(bad - ref.ig) > VISIBLE * ref.budget
    can_move = np.asarray(ref.d) != 0
    if fault == "stale_sum":                               # rows of the first block have nothing stale to add
        can_move = can_move & (np.arange(c.n)[:, None] >= c.max_batch)
        assert not out[:c.max_batch].any()
    print("%s b=%.2f %s: %.3f of the live cells leave %g budgets (%.3f can move)" % (name, baseline, fault, out.mean(), VISIBLE, can_move.mean()))
    assert can_move.mean() > 0.1
    assert out.sum() >= SHARE * can_move.sum()


def test_a_missing_input_derivative_cannot_show_inside_the_domain(oracle_mod):
    """f' left out of g: inside the device call's domain the fault moves NO cell -- f is the identity on the non-negative points,
    so f'(a_k) = 1 wherever a_k > 0, and a_k = 0 needs x0 = b_f = 0, where d = 0 -- and the device test cannot see it either.  The
    product's factor f' is pinned by the input-gradient suites (tests/test_input_gradient_cpu.py: wrong_rule_prime); here the
    fault model is shown to bite where it can, on the host route's wider domain: the same fixtures behind a sigmoid or tanh."""
    for name in F32:
        c = ac.BY_NAME[name]
        X, Y = ac.rows(c)
        for baseline in ic.BASELINES:
            ref = ic.reference(oracle_mod, c, baseline)
            bad = ic.model(ac.weights(oracle_mod, c), X, Y, c.inner, ic.STEPS, baseline, False, "no_fprime").ig
            assert np.array_equal(bad, ref.ig), (name, baseline)
    for inner in (ac.SIGMOID, ac.TANH):
        c = ac.BY_NAME["ident"]._replace(inner=inner)
        X, Y = ac.rows(c)
        Ws = ac.weights(oracle_mod, c)
        for baseline in ic.BASELINES:
            ref = ic.model(Ws, X, Y, inner, ic.STEPS, baseline)
            budget = ic.element_budget(ref.d, ref.gs, ref.ig)
            bad = ic.model(Ws, X, Y, inner, ic.STEPS, baseline, False, "no_fprime").ig
            out = np.abs(bad - ref.ig) > VISIBLE * budget
            print("inner %d b=%.2f no_fprime: %.3f of the live cells leave %g budgets" % (inner, baseline, out.mean(), VISIBLE))
            assert out.sum() >= SHARE * (np.asarray(ref.d) != 0).sum()


@pytest.mark.parametrize("baseline", ic.BASELINES)
@pytest.mark.parametrize("name", F32)
def test_completeness_gap_of_the_model(oracle_mod, name, baseline):
    """recorded: the fp64 model's gap at 8 and 32 points and the left-endpoint rule's at 8 (the table above).  On a path without
    kinks the midpoint rule is second order: 32 points for 8 cut the gap more than tenfold (1 / m^2: sixteenfold) and the
    left-endpoint rule is at least 100 times worse.  Across kinks both rules are first order: the figures are recorded, and the
    gap must still fall with m."""
    c = ac.BY_NAME[name]
    g8 = float(np.abs(ic.model_gap(oracle_mod, c, baseline)).max())
    g32 = float(np.abs(ic.model_gap(oracle_mod, c, baseline, ic.MORE_STEPS)).max())
    left = float(np.abs(ic.model_gap(oracle_mod, c, baseline, rule="left")).max())
    rows = float(ic.reference(oracle_mod, c, baseline).budget.sum(axis=1).max())
    print("%s b=%.2f: gap at %d points %.3g, at %d points %.3g (%.1f x), left-endpoint rule %.3g (%.0f x); a row's budgets sum to %.3g at most"
          % (name, baseline, ic.STEPS, g8, ic.MORE_STEPS, g32, g8 / g32, left, left / g8, rows))
    assert g8 > 0 and g32 < g8
    if kink_free(c, baseline):
        assert left >= 100 * g8
        assert g32 * 10 <= g8
    else:
        assert g32 * 2 <= g8
        assert left >= g8
