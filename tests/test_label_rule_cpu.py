"""The fixtures of tests/test_label_rule_gpu.py are what they claim to be, and its comparisons have teeth: on every fixture
the fp64 oracles (f32: np_oracle.forward; bf16: forward_bf16, also under the saturation tests' jitter seeds) show every planned
group on top, the regimes mixed in every 4-row block and 16-row group, a lead of the winning group of at least 100 output
budgets, and the labels of the reference's scan; numpy models of the heads' lane geometries (tests/label_rule_cases.py) give the
same labels when they are right, and each fault model L1 .. L10 that can occur in a geometry moves at least one label, the
hit count and the confusion matrix.  No GPU."""
import numpy as np
import pytest

from tests import label_rule_cases as lc
from tests import saturation_cases as sc

DTYPES = ((lc.F32, "f32"), (lc.BF16, "bf16"))


def _truths(fx, dtype):
    """The dtype's truth, and for bf16 the truths under jitter (another summation order before the bf16 rounding)."""
    out = [fx.truth(dtype)]
    if dtype == lc.BF16:
        out += [lc.Truth(fx, dtype, jitter=(sc.JITTER, np.random.default_rng(seed))) for seed in sc.JITTER_SEEDS]
    return out


@pytest.mark.parametrize("name", lc.NAMES)
def test_the_construction(oracle_mod, name):
    fx = lc.fixture(oracle_mod, name)
    n, G, Lm = fx.dims[-1], len(fx.groups), len(fx.dims) - 1
    assert np.array_equal(fx.X, sc.f32(fx.X), equal_nan=True) and np.array_equal(fx.w, sc.f32(fx.w))   # what the device holds
    assert G >= 4 and any(len(g) == 3 for g in fx.groups)
    for l in range(Lm - 1):                                     # the selectors: nothing else in or out
        for u in range(G + 1):
            assert fx.Ws[l][u, u] > 0 and np.count_nonzero(fx.Ws[l][u, :]) == 1 and np.count_nonzero(fx.Ws[l][:, u]) == 1
    last = fx.Ws[Lm - 1]
    for gi, g in enumerate(fx.groups):
        assert all(np.array_equal(last[:, j], last[:, g[0]]) for j in g)                  # identical columns
        assert (last[gi, list(g)] == fx.c).all() and np.count_nonzero(last[gi]) == len(g)
    assert (last[G] == -fx.d).all() and fx.c > 0 and fx.d > 0
    assert len({last[:, j].tobytes() for j in fx.reps}) == len(fx.reps)                   # and no other two alike
    # the regimes: every 4-row block and 16-row group mixed, a NaN row in every 16-row group
    for size in (4, 16):
        for b in range(0, fx.rows, size):
            blk = fx.regime[b:b + size]
            assert len(blk) < 3 or len(set(blk)) >= 3, (size, b)
            assert size == 4 or len(blk) < 5 or lc.R_NAN in blk
    for g in range(G):
        assert ((fx.regime == g) | ((fx.regime == lc.R_DOWN) & (fx.top == g))).sum() >= 2
    assert (fx.regime == lc.R_NAN).sum() >= 2 and fx.has_tie == ((fx.regime == lc.R_TIE).sum() >= 2)
    assert fx.has_down == ((fx.regime == lc.R_DOWN).sum() >= 2)
    # expected rows: one-hot; hits and misses on the rows with a group on top
    assert ((fx.Y == 0) | (fx.Y == 1)).all() and (fx.Y.sum(axis=1) == 1).all()
    want = lc.expected_class(fx.Y)
    on_top = fx.regime >= 0
    hi = np.array([fx.groups[t][-1] for t in fx.top])
    lo = np.array([fx.groups[t][0] for t in fx.top])
    assert ((want == hi) | (want == lo))[on_top | (fx.regime == lc.R_DOWN)].all()
    assert (want == hi)[on_top].sum() > (want == lo)[on_top].sum() > 0
    assert set(want[fx.regime == lc.R_NAN]) == {0, n - 1}


@pytest.mark.parametrize("name", lc.NAMES)
def test_rows_and_leads(oracle_mod, name):
    fx = lc.fixture(oracle_mod, name)
    n = fx.dims[-1]
    relu_down = fx.out_kind == lc.GENERAL and fx.last == lc.RELU
    for dtype, dname in DTYPES:
        leads = []
        for t in _truths(fx, dtype):
            for i in range(fx.rows):
                r, out = fx.regime[i], t.out[i]
                if r == lc.R_NAN and relu_down:                           # relu(NaN) = 0
                    assert (out == 0).all() and t.label[i] == n - 1
                elif r == lc.R_NAN:
                    assert np.isnan(out).all() and t.label[i] == 0
                elif r == lc.R_TIE or (r == lc.R_DOWN and relu_down):
                    assert (out == out[0]).all() and t.label[i] == n - 1
                    assert r == lc.R_TIE or (out == 0).all()
                else:
                    g = fx.groups[fx.top[i]]
                    assert t.label[i] == g[-1] and (out[list(g)] == out[g[0]]).all()
                    if r == lc.R_DOWN and (fx.out_kind == lc.SCE or fx.last in (lc.IDENT, lc.LEAKY)):
                        assert (t.key[i] < 0).all()                       # the rows a padding column's 0 would win
                assert t.label[i] == oracle_mod.argmax_rule(out)          # the C oracle's scan on the expanded row
            assert np.array_equal(t.label, fx.truth(dtype).label)        # (jitter moves no label)
            for b in range(0, fx.rows, 4):                                # beside every NaN row a label that is not 0
                if lc.R_NAN in fx.regime[b:b + 4] and len(fx.regime[b:b + 4]) > 1 and not relu_down:
                    assert t.label[b:b + 4].max() > 0
            # each group on top (label = its highest index) in at least two rows
            for g in fx.groups:
                assert (t.label[fx.regime != lc.R_TIE] == g[-1]).sum() >= 2 or g[-1] == n - 1 and (t.label == g[-1]).sum() >= 2
            leads.append(lc.lead_in_budgets(fx, t, dtype))
            # in f32 the winning group stays apart from the rest (a saturating last activation must not merge them at 1.0)
            k32 = t.key.astype(np.float32)
            for i in np.flatnonzero(fx.regime >= 0):
                g = list(fx.groups[fx.top[i]])
                assert k32[i, g[0]] > np.delete(k32[i], g).max()
        print("%s %s: c = %.6g, d = %.6g, smallest lead %.0f budgets (%.3g)" % (name, dname, fx.c, fx.d, min(leads), min(leads) * lc.BUDGET[dtype]["p"]))
        assert min(leads) >= lc.MIN_LEAD_BUDGETS
    # the C oracle on host rows: the whole matrix, sample by sample
    ref = oracle_mod.OracleNet(fx.dims, out_kind=fx.out_kind, inner_act=fx.inner, last_act=fx.last)
    ref.set_weights(fx.w)
    assert np.array_equal(ref.argmax(fx.X), fx.truth(lc.F32).label)
    for v in fx.nan_cols:
        ref.set_weights(fx.variant(v))
        assert np.array_equal(ref.argmax(fx.X), fx.truth(lc.F32, v).label), v
    ref.close()


@pytest.mark.parametrize("name", lc.NAMES)
def test_column_nan_variants(oracle_mod, name):
    fx = lc.fixture(oracle_mod, name)
    relu_last = fx.out_kind == lc.GENERAL and fx.last == lc.RELU
    for dtype, _ in DTYPES:
        base = fx.truth(dtype)
        for v, col in fx.nan_cols.items():
            t = fx.truth(dtype, v)
            assert np.isnan(t.Z[:, col]).all()
            if relu_last and v != "hi":                                   # relu(NaN) = 0: a column of zeros, which wins no row it did not
                assert not np.isnan(t.out).any() and np.array_equal(t.label, base.label)
                continue
            if v in ("nan", "col0"):
                assert (t.label == 0).all()
            elif v == "single":
                assert np.array_equal(t.label, base.label) and not np.isnan(t.out[fx.regime != lc.R_NAN]).all(axis=1).any()
            else:
                g = fx.groups[fx.hi_group]
                moved = (fx.top == fx.hi_group) & (fx.regime != lc.R_NAN) & ~((fx.regime == lc.R_DOWN) & (fx.last == lc.RELU))
                assert moved.sum() >= 2 and (t.label[moved] == g[-2]).all() and (base.label[moved] == g[-1]).all()
                assert np.array_equal(t.label[~moved], base.label[~moved])
            if v != "single":
                assert t.hits != base.hits and not np.array_equal(t.conf, base.conf)


def _moves(fx, t, labels):
    return (not np.array_equal(labels, t.label), lc.hits_of(labels, fx.Y) != t.hits,
            not np.array_equal(lc.confusion_of(labels, fx.Y)[:, :-1], t.conf) or bool(lc.confusion_of(labels, fx.Y)[:, -1].any()))


@pytest.mark.parametrize("name", lc.NAMES)
def test_the_right_models_agree_and_every_fault_shows(oracle_mod, name):
    fx = lc.fixture(oracle_mod, name)
    softmax = fx.out_kind == lc.SCE
    for dtype, dname in DTYPES:
        caught = {}
        for geom in lc.geometries_for(fx):
            for v in (None,) + tuple(fx.nan_cols):                       # a right head of every geometry gives the truth
                t = fx.truth(dtype, v)
                assert np.array_equal(lc.head_labels(t.key, geom, softmax), t.label), (geom, v)
            for fault in lc.faults_for(fx, geom):
                for v in lc.FAULT_VARIANTS.get(fault, (None,)):
                    t = fx.truth(dtype, v)
                    moved = _moves(fx, t, lc.head_labels(t.key, geom, softmax, **lc.FAULTS[fault]))
                    assert all(moved), (name, dname, geom, fault, v, moved)
                caught.setdefault(geom, []).append(fault)
        print("%s %s catches: %s" % (name, dname, "; ".join("%s %s" % (g, " ".join(f)) for g, f in caught.items())))


@pytest.mark.parametrize("name", lc.GROUP_NAMES)
def test_the_ensemble_scan(oracle_mod, name):
    """group_combine_kernel scans the member-order f32 mean of the members' probabilities: ties are exact because each member's
    duplicate columns are, and L10 (the scan with `>`) shows."""
    members = [lc.fixture(oracle_mod, name, seed) for seed in lc.GROUP_SEEDS]
    fx = members[0]
    for m in members[1:]:
        assert np.array_equal(m.X, fx.X, equal_nan=True) and m.Y is fx.Y and m.groups == fx.groups and not np.array_equal(m.w, fx.w)
    for dtype, dname in DTYPES:
        mean, label, hits, conf = lc.ensemble_truth(members, dtype)
        for g in fx.groups:
            assert (mean[:, list(g)] == mean[:, [g[0]]])[fx.regime != lc.R_NAN].all()
        assert np.array_equal(label, fx.truth(dtype).label)            # every member puts the same group on top
        assert np.array_equal(lc.head_labels(mean, "serial", False), label)
        # the lead of the winning group in the mean probability
        lead = min((mean[i, fx.groups[fx.top[i]][0]] - np.delete(mean[i], list(fx.groups[fx.top[i]])).max()) / lc.BUDGET[dtype]["p"]
                   for i in range(fx.rows) if fx.regime[i] >= 0 or fx.regime[i] == lc.R_DOWN)
        print("%s %s ensemble: smallest lead %.0f budgets; catches L10" % (name, dname, lead))
        assert lead >= 50.0   # (a three-way group's members hold 1/3 each: 67 bf16 budgets is all a probability can lead by)
        bad = lc.head_labels(mean, "serial", False, **lc.FAULTS["L10"])
        assert not np.array_equal(bad, label) and lc.hits_of(bad, fx.Y) != hits
        assert not np.array_equal(lc.confusion_of(bad, fx.Y)[:, :-1], conf)
        # one member with a NaN weight: its rows are all 0, and so is the ensemble
        _, label_n, hits_n, _ = lc.ensemble_truth(members, dtype, nan_member=1)
        assert (members[1].truth(dtype, "nan").label == 0).all() and (label_n == 0).all() and hits_n != hits


def test_every_head_has_a_route():
    """Bookkeeping over the GPU file's route table (no device): which head a route reaches follows from the plan rules, as in
    tests/test_saturation_cpu.py::test_every_head_has_a_shift_and_a_spread_route; a softmax net of more than 16 and at most
    1024 padded outputs on the per-layer path goes to output_layer_kernel's register arm (plan.hip use_tail, kernels.h)."""
    from tests import test_label_rule_gpu as tg
    assert {r[0] for r in tg.ROUTES} == set(lc.NAMES)
    heads = {False: set(), True: set()}
    for name, dt, env, route in tg.ROUTES:
        _, dims, out_kind = next(x for x in lc._TABLE if x[0] == name)[:3]
        small, out = dims[-1] <= 16, heads[out_kind == lc.GENERAL]
        if route == "static":
            out.add("static-bf16" if dt else "static-f32")
        elif route == "rb":
            # (f32: middle4's forward-only instance; bf16: per-layer GEMMs + tail_kernel<BF16>, or the output kernel's element-wise arm)
            out.add(("tail-bf16" if out_kind == lc.SCE else "output-elementwise") if dt else "middle4-rowtail")
        elif route == "m4":
            out.add("middle4-rowtail" if small and dims[-2] <= 128 else "middle4-register" if small else "middle4-general")
        elif out_kind == lc.GENERAL:
            out.add("output-elementwise")
        elif env == tg.GENERIC and small:
            out.add("tail-bf16" if dt else "tail-f32")
        elif env == tg.NO_TAIL:
            out.add("output-register")
        else:
            out.add("output-three-pass" if dims[-1] > 1024 else "output-register-two-chunks")
    assert heads[False] == {"static-f32", "static-bf16", "middle4-rowtail", "middle4-register", "middle4-general", "tail-f32", "tail-bf16",
                            "output-register", "output-register-two-chunks", "output-three-pass"}
    assert heads[True] == {"static-f32", "static-bf16", "middle4-rowtail", "middle4-general", "output-elementwise"}
    assert set(tg.GROUPS_F) == {(n, d) for n in lc.GROUP_NAMES for d in (lc.F32, lc.BF16)}
