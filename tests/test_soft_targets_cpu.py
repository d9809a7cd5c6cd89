"""The fixtures of tests/test_soft_targets_gpu.py are what they claim to be, and its comparisons have teeth (fixtures, budgets
and fault models: tests/soft_target_cases.py).  Established from the oracles, before any device run:
  1. a plain float32 restatement of the reference's formulas stays inside a QUARTER of every budget on every fixture (outputs,
     per-row loss, every gradient element, W and V after the steps); bf16: np_oracle's jittered bf16 oracle (1e-6, four seeds)
     against the unjittered one;
  2. every fault model leaves the budget of its dtype by a factor of FOUR or more, in the loss of at least one row or in the
     gradient, on every fixture where it can occur (targets narrowed to bf16: required on the f32 nets, reported on the bf16 ones);
  3. all six target kinds occur, every 4-row block holds three or more, every 16-row group all six;
  4. by the expected-class rule (MT:186-188: the last exact 1.0, else class 0) hits and misses fall on rows that are not one-hot,
     and the count is decided by top-2 margins above the project's on 80 % of the rows or more.
No GPU."""
import numpy as np
import pytest

from tests import np_oracle
from tests import soft_target_cases as st

DT = {st.F32: "f32", st.BF16: "bf16"}


@pytest.mark.parametrize("name", st.NAMES)
def test_fixtures_are_f32_exact_and_the_c_oracle_agrees(oracle_mod, name):
    fx = st.fixture(oracle_mod, name)
    t = fx.truth(st.F32)
    for a in (fx.X, fx.Y, fx.Xh, fx.Yh, fx.w):
        assert np.array_equal(a, st.f32(a))                      # what the device holds, exactly
    assert fx.X.shape == (fx.rows, fx.dims[0]) and fx.Y.shape == (fx.rows, fx.dims[-1])
    assert ((fx.X == 0).mean() > 0.4) and ((fx.X == 0).mean() < 0.6)
    ref = oracle_mod.OracleNet(fx.dims, out_kind=fx.out_kind, inner_act=fx.inner, last_act=fx.last)
    ref.set_alloc_per_sample(0)
    ref.set_weights(fx.w)
    assert np.abs(ref.propagate(fx.X) - t.out).max() <= 1e-9 * max(1.0, np.abs(t.out).max())
    assert np.allclose(ref.calculate_loss(fx.X, fx.Y), t.loss, rtol=1e-9, atol=1e-9 * t.terms.max())
    G = sum(ref.calculate_weight_gradient(x, y) for x, y in zip(fx.X, fx.Y))      # (one sample per call)
    assert np.abs(G - t.G).max() <= 1e-9 * np.abs(t.G).max()
    ref.gradient_step(fx.X, fx.Y, st.STEP, st.MOMENTUM)
    ref.gradient_step(fx.X, fx.Y, st.STEP, st.MOMENTUM)
    assert np.abs(ref.get_weights() - t.w).max() <= 1e-9 and np.abs(ref.get_momentum() - t.v).max() <= 1e-9
    ref.close()
    print(name, "max |z| %.2f, loss %.3g .. %.3g" % (np.abs(t.Z).max(), t.loss.min(), t.loss.max()))
    if fx.out_kind == st.SCE:
        lo, hi = (0.3, 1.0) if name == "TB" else (1.0, 6.0)       # logits of order one to three (TB: 784 inputs, drawn lower: 0.52)
        assert lo <= np.abs(t.Z).max() <= hi, np.abs(t.Z).max()


@pytest.mark.parametrize("name", st.NAMES)
def test_target_kinds(oracle_mod, name):
    fx = st.fixture(oracle_mod, name)
    Y, kind, d = fx.Y, fx.kind, fx.dims[-1]
    bf = np_oracle.bf16_round(Y)
    assert np.array_equal(kind, st.kinds(fx.rows, fx.out_kind))
    for Yx, kx in ((Y, kind), (fx.Yh, st.kinds(st.HELD_ROWS, fx.out_kind))):
        for r, k in enumerate(kx):
            y = Yx[r]
            if k == st.SMOOTHED:
                assert (y > 0).all() and abs(y.sum() - 1) < 1e-6 and np.isclose(y.max(), 0.9) and (np.sort(y)[:-1] == y.min()).all()
            elif k == st.TEACHER:
                assert (y > 0).all() and abs(y.sum() - 1) < 1e-6 and (y < 1).all()
            elif k == st.TWO_ONES:
                assert (y == 1.0).sum() == 2 and y.sum() == 2.0
            elif k == st.ZERO:
                assert (y == 0).all()
            elif k == st.FREE:
                assert y.min() < 0 and y.max() > 1 and abs(y.sum() - 1) > 0.05 and y.min() >= -0.5 and y.max() <= 1.5
            else:
                assert (y == 1.0).sum() == 1 and y.sum() == 1.0
    for k in (st.SMOOTHED, st.TEACHER, st.FREE):                 # values bf16 cannot hold, on every such row
        for r in np.flatnonzero(kind == k):
            assert (bf[r] != Y[r]).any(), (name, r)
    if fx.out_kind == st.SCE:
        assert set(kind) == set(range(st.N_KINDS))
        assert (kind == st.TWO_ONES).any() and (kind == st.ZERO).any()
        assert all(len(set(kind[g:g + 4])) >= min(3, len(kind[g:g + 4])) for g in range(0, fx.rows, 4))
        assert all(len(set(kind[g:g + 16])) == st.N_KINDS for g in range(0, fx.rows, 16) if len(kind[g:g + 16]) >= st.N_KINDS)
    else:
        assert set(kind) == {st.FREE, st.ONE_HOT} and all(len(set(kind[g:g + 4])) == 2 for g in range(0, fx.rows - 1, 4))


@pytest.mark.parametrize("name", st.NAMES)
def test_the_float32_restatement_stays_within_a_quarter_of_every_budget(oracle_mod, name):
    fx = st.fixture(oracle_mod, name)
    t, r = fx.truth(st.F32), st.Restated(fx)
    used = dict(out=np.abs(r.out - t.out).max() / st.out_bound(fx, st.F32, t.out),
                loss=st.loss_distance(fx, st.F32, r.loss, t),
                gradient=st.gradient_distance(fx, st.F32, r.G, t.G),
                W=np.abs(r.w - t.w).max() / st.weight_bound(st.F32), V=np.abs(r.v - t.v).max() / st.weight_bound(st.F32))
    print(name, "float32 restatement, fraction of the f32 budgets:", {k: "%.4f" % v for k, v in used.items()})
    assert max(used.values()) <= 0.25, used
    # bf16: the oracle under jitter (another summation order of the f32 sums before their bf16 rounding) against itself
    tb = fx.truth(st.BF16)
    worst = dict(out=0.0, loss=0.0, gradient=0.0, W=0.0, V=0.0)
    for seed in st.JITTER_SEEDS:
        tj = st.Truth(fx, st.BF16, jitter=(st.JITTER, np.random.default_rng(seed)))
        worst["out"] = max(worst["out"], np.abs(tj.out - tb.out).max() / st.out_bound(fx, st.BF16, tb.out))
        worst["loss"] = max(worst["loss"], st.loss_distance(fx, st.BF16, tj.loss, tb))
        worst["gradient"] = max(worst["gradient"], st.gradient_distance(fx, st.BF16, tj.G, tb.G))
        worst["W"] = max(worst["W"], np.abs(tj.w - tb.w).max() / st.weight_bound(st.BF16))
        worst["V"] = max(worst["V"], np.abs(tj.v - tb.v).max() / st.weight_bound(st.BF16))
    print(name, "bf16 oracle under jitter, fraction of the bf16 budgets:", {k: "%.4f" % v for k, v in worst.items()})
    assert max(worst.values()) <= 0.25, worst


def _occurs(fx, model):
    """A model can occur where the fixture has a row it treats differently (every model does on the six kinds; the General
    fixtures have no softmax loss expression)."""
    return model in (st.SOFTMAX_FAULTS if fx.out_kind == st.SCE else st.GENERAL_FAULTS)


@pytest.mark.parametrize("name", st.NAMES)
def test_every_fault_model_leaves_the_budget_by_a_factor_of_four(oracle_mod, name):
    fx = st.fixture(oracle_mod, name)
    for dtype in (st.F32, st.BF16):
        t = fx.truth(dtype)
        # the truth itself is at distance 0, and a model is judged on the dtype's own logits: the distance is the model's alone
        assert st.loss_distance(fx, dtype, t.loss, t) == 0.0
        for model in st.SOFTMAX_FAULTS:
            if not _occurs(fx, model):
                continue
            loss, G = st.faulty(fx, dtype, model)
            dl = st.loss_distance(fx, dtype, loss, t)
            dg = None if G is None else st.gradient_distance(fx, dtype, G, t.G)
            required = not (model == "ybf16" and dtype == st.BF16)
            print("%s %s %-12s loss %9.3g budgets%s%s" % (name, DT[dtype], model, dl, "" if dg is None else ", gradient %9.3g budgets" % dg,
                                                         "" if required else "  (reported, not required)"))
            if required:
                assert max(dl, dg or 0.0) >= 4.0, (name, DT[dtype], model, dl, dg)
                if model in st.LOSS_FAULTS or dtype == st.F32:    # the loss alone shows every model of the loss expression, and on f32 nets every model
                    assert dl >= 4.0, (name, DT[dtype], model, dl)
                if dg is not None:                                # a wrong target row in the delta shows in the gradient
                    assert dg >= 4.0, (name, DT[dtype], model, dg)


@pytest.mark.parametrize("name", st.SOFTMAX)
def test_hits_and_misses_fall_on_rows_that_are_not_one_hot(oracle_mod, name):
    fx = st.fixture(oracle_mod, name)
    soft = fx.kind != st.ONE_HOT
    assert np.array_equal(st.expected_class(fx.Y)[fx.kind == st.TWO_ONES], [np.flatnonzero(y == 1.0)[-1] for y in fx.Y[fx.kind == st.TWO_ONES]])
    assert (st.expected_class(fx.Y)[np.isin(fx.kind, (st.SMOOTHED, st.TEACHER, st.ZERO, st.FREE))] == 0).all()
    for dtype in (st.F32, st.BF16):
        t = fx.truth(dtype)
        hit = t.label == t.expected
        lo, hi = t.hits_bounds()
        print(name, DT[dtype], "safe rows %d of %d, hits in [%d, %d], on soft rows %d hits and %d misses"
              % (t.safe.sum(), fx.rows, lo, hi, (hit & soft & t.safe).sum(), (~hit & soft & t.safe).sum()))
        assert t.safe.mean() >= 0.8
        assert (hit & soft & t.safe).any() and (~hit & soft & t.safe).any()
        assert np.array_equal(t.label[t.safe], fx.truth(st.F32).label[t.safe])
    # a head that took the argmax of the row for its expected class would count otherwise
    assert (fx.Y.argmax(axis=1) != st.expected_class(fx.Y)).any()


@pytest.mark.parametrize("dtype", [st.F32, st.BF16], ids=["f32", "bf16"])
def test_the_held_out_best_point_is_decided_by_more_than_the_budget(oracle_mod, dtype):
    """train_sampled_held_out(rule="loss") on T4: the lowest loss sum lies below every other point's by more than twice both
    points' summed per-row budgets (both may err by their whole budget towards each other and half the gap remains)."""
    fx = st.fixture(oracle_mod, "T4")
    loss, bound, hits = st.held_out_curve(oracle_mod, fx, dtype)
    best = int(loss.argmin())
    print("T4", DT[dtype], "held-out loss sums", loss.tolist(), "bounds", bound.tolist(), "hits", hits, "best point", best)
    assert len(loss) == st.HELD["iterations"] // st.HELD["every"] == 3
    for p in range(len(loss)):
        if p != best:
            assert loss[p] - loss[best] > 2.0 * (bound[p] + bound[best]), (p, best)
    assert set(st.kinds(st.HELD_ROWS)) == set(range(st.N_KINDS))
