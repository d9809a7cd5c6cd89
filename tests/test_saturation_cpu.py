"""The fixtures of tests/test_saturation_gpu.py are what they claim to be, and its comparisons have teeth: on every fixture the
fp64 oracles show the row classes / the spread, a CORRECT numpy-f32 max-subtracted head stays within a quarter of the probability
and loss budgets (also from f32-rounded last hidden activations; bf16: under np_oracle's jitter, four seeds), and every fault
model of tests/saturation_cases.py that applies leaves the budgets (NaN and inf count as leaving).  No GPU."""
import numpy as np
import pytest

from tests import np_oracle
from tests import saturation_cases as sc


def _groups_mixed(cls, size):
    return all(len(set(cls[g:g + size])) >= 2 for g in range(0, len(cls), size) if len(cls[g:g + size]) >= 2)


@pytest.mark.parametrize("name", sc.NAMES)
def test_row_classes_and_spread(oracle_mod, name):
    fx = sc.fixture(oracle_mod, name)
    t = fx.truth(sc.F32)
    assert np.array_equal(fx.X, sc.f32(fx.X)) and np.array_equal(fx.w, sc.f32(fx.w))   # what the device holds, exactly
    ref = oracle_mod.OracleNet(fx.dims, out_kind=fx.out_kind, inner_act=fx.inner, last_act=fx.last)
    ref.set_weights(fx.w)
    zc = ref.logits(fx.X)                                                            # the C oracle agrees on the logits
    assert np.abs(zc - t.Z).max() <= 1e-9 * np.abs(t.Z).max()
    ref.close()
    if fx.kind == "shift":
        z = t.Z
        assert (z[fx.cls == sc.HIGH] >= 100.0).all() and (z[fx.cls == sc.LOW] <= -100.0).all()
        assert (np.abs(z[fx.cls == sc.NEUTRAL]) <= 40.0).all()
        assert np.array_equal(fx.cls, np.arange(fx.rows) % 3)
        assert _groups_mixed(fx.cls, 4) and _groups_mixed(fx.cls, 16)
        Lm = len(fx.dims) - 1
        for l in range(Lm - 1):                                                      # the chain: nothing else in or out
            for u in (sc.UP, sc.UM):
                assert fx.Ws[l][u, u] > 0 and np.count_nonzero(fx.Ws[l][u, :]) == 1 and np.count_nonzero(fx.Ws[l][:, u]) == 1
        assert (fx.Ws[Lm - 1][sc.UP] == fx.c).all() and (fx.Ws[Lm - 1][sc.UM] == -fx.c).all()
        print(name, "c = %.6g, high rows min %.1f, low rows max %.1f, neutral max |z| %.1f"
              % (fx.c, z[fx.cls == sc.HIGH].min(), z[fx.cls == sc.LOW].max(), np.abs(z[fx.cls == sc.NEUTRAL]).max()))
    else:
        s = np.sort(t.Z, axis=1)
        gap = s[:, -1] - s[:, -2]
        assert (gap >= 110.0).mean() >= 0.5 and np.abs(t.Z).max() <= 300.0
        odd = np.arange(fx.rows) % 2 == 1
        assert (t.loss[odd] >= 100.0).all() and (t.loss[odd] <= 300.0).all() and (t.loss[~odd] <= 1e-40).all()
        p32, _ = sc.head_correct(t.Z, fx.Y)
        assert ((p32 * fx.Y).sum(axis=1)[~odd] == 1.0).all() and ((p32 * fx.Y).sum(axis=1)[odd] == 0.0).all()
        print(name, "top-2 gap %.1f .. %.1f, max |z| %.1f, odd-row loss %.1f .. %.1f" % (gap.min(), gap.max(), np.abs(t.Z).max(), t.loss[odd].min(), t.loss[odd].max()))


@pytest.mark.parametrize("name", sc.SOFTMAX_SHIFT + sc.SPREAD)
def test_the_correct_head_stays_within_a_quarter_of_the_budgets(oracle_mod, name):
    fx = sc.fixture(oracle_mod, name)
    t = fx.truth(sc.F32)
    ep, el = sc.in_budget(*sc.head_correct(t.Z, fx.Y), t, sc.F32, 0.25)
    print(name, "f32 head on fp64 logits: %.3f / %.3f of a quarter budget" % (ep, el))
    assert ep <= 1.0 and el <= 1.0
    # ... from last hidden activations rounded to f32
    Z, _ = np_oracle.forward(fx.Ws, fx.X, fx.inner, fx.out_kind, fx.last)
    z32 = sc.f32(np_oracle.act(fx.inner, Z[-2])) @ fx.Ws[-1]
    ep, el = sc.in_budget(*sc.head_correct(z32, fx.Y), t, sc.F32, 0.25)
    print(name, "  ... f32-rounded last hidden activations: %.3f / %.3f" % (ep, el))
    assert ep <= 1.0 and el <= 1.0
    # bf16: the oracle under jitter (another summation order of the f32 sums before their bf16 rounding), the f32 head on top
    tb = fx.truth(sc.BF16)
    worst = 0.0
    for seed in sc.JITTER_SEEDS:
        tj = sc.Truth(fx, sc.BF16, jitter=(sc.JITTER, np.random.default_rng(seed)))
        ep, el = sc.in_budget(*sc.head_correct(tj.Z, fx.Y), tb, sc.BF16, 0.25)
        worst = max(worst, ep, el)
    print(name, "  ... bf16 under jitter: %.3f of a quarter budget" % worst)
    assert worst <= 1.0   # (no spread fixture had to be dropped for bf16)


@pytest.mark.parametrize("name", sc.SOFTMAX_SHIFT)
def test_max_faults_leave_the_budgets_on_shift_fixtures(oracle_mod, name):
    fx = sc.fixture(oracle_mod, name)
    for dtype in (sc.F32, sc.BF16):
        t = fx.truth(dtype)
        for fault, head in sc.SHIFT_FAULTS.items():
            if fault == "F2" and fx.dims[-1] % 16 == 0:
                continue                                     # no padding column
            if fault == "F3'" and fx.rows <= 16 and len(set(fx.cls[:16])) < 2:
                continue
            ep, el = sc.in_budget(*head(t.Z, fx.Y), t, dtype)
            assert max(ep, el) > 1.0, (name, fault, ep, el)
        # a head that is right must not: the models differ from it in the maximum alone
        assert max(sc.in_budget(*sc.head_correct(t.Z, fx.Y), t, dtype)) <= 1.0


@pytest.mark.parametrize("name", sc.SPREAD)
def test_log_p_leaves_the_budget_on_spread_fixtures(oracle_mod, name):
    fx = sc.fixture(oracle_mod, name)
    for dtype in (sc.F32, sc.BF16):
        t = fx.truth(dtype)
        ep, el = sc.in_budget(*sc.head_f4_log_p(t.Z, fx.Y), t, dtype)
        assert ep <= 1.0 and el > 1.0, (name, ep, el)


def test_exp_over_one_plus_exp_leaves_the_budget_on_saturated_sigmoid_outputs(oracle_mod):
    fx = sc.fixture(oracle_mod, "G_sigm")
    t = fx.truth(sc.F32)
    assert np.abs(sc.sigmoid_f32(t.Z) - t.out).max() <= 2e-5
    with np.errstate(all="ignore"):
        bad = np.abs(sc.sigmoid_f6(t.Z) - t.out)
    assert not (bad <= 2e-5).all() and np.isnan(bad[fx.cls == sc.HIGH]).all()


@pytest.mark.parametrize("name", sc.GENERAL_NAMES)
def test_general_outputs_are_saturated(oracle_mod, name):
    fx = sc.fixture(oracle_mod, name)
    t = fx.truth(sc.F32)
    hi, lo = t.out[fx.cls == sc.HIGH], t.out[fx.cls == sc.LOW]
    if fx.last == sc.IDENT:
        assert (hi >= 100).all() and (lo <= -100).all()
    elif fx.last == sc.LEAKY:
        assert (hi >= 100).all() and (lo <= -1).all() and (lo >= -3).all()
    elif fx.last == sc.RELU:
        assert (hi >= 100).all() and (lo == 0).all()
    elif fx.last == sc.SIGMOID:
        assert (hi.astype(np.float32) == 1).all() and (lo <= 1e-40).all()
    else:
        assert (hi.astype(np.float32) == 1).all() and (lo.astype(np.float32) == -1).all()
    assert np.isfinite(t.G).all() and np.isfinite(t.w).all()


@pytest.mark.parametrize("name", sc.SOFTMAX_SHIFT + sc.SPREAD)
def test_labels_are_safe_on_nearly_every_row(oracle_mod, name):
    fx = sc.fixture(oracle_mod, name)
    for dtype in (sc.F32, sc.BF16):
        t = fx.truth(dtype)
        print(name, "bf16" if dtype else "f32", "safe rows %d of %d" % (t.safe.sum(), fx.rows))
        assert t.safe.mean() >= 0.9
        assert np.array_equal(t.label[t.safe], fx.truth(sc.F32).label[t.safe])


@pytest.mark.parametrize("name", sc.NAMES)
def test_the_widened_entries_are_the_chain_columns_alone(oracle_mod, name):
    fx = sc.fixture(oracle_mod, name)
    Lm = len(fx.dims) - 1
    assert all(len(c) <= 2 for c in fx.chain_cols.values()) and all(l < Lm - 1 for l in fx.chain_cols)
    for dtype in (sc.F32, sc.BF16):
        t = fx.truth(dtype)
        b = sc.BUDGET[dtype]
        want_g, want_w = sc.widened_entries(fx, t.w)
        if fx.kind == "shift":
            assert want_w[Lm - 1] == 2 * fx.dims[-1]
        noise = sc.chain_noise(fx, dtype)
        print(name, "bf16" if dtype else "f32", "chain-column gradient noise per layer:", {l: "%.3g" % v for l, v in noise.items()})
        assert all(np.isfinite(v) for v in noise.values())
        G = np_oracle.split(t.G, fx.dims)
        for l, tol in enumerate(sc.gradient_bounds(fx, dtype, t.G)):
            base = b["g"] * np.abs(G[l]).max() + b["g_abs"]
            wide = tol != base
            assert wide.sum() <= want_g.get(l, 0) and (tol >= base).all()
            if wide.any():
                assert set(np.flatnonzero(wide.any(axis=0))) <= set(fx.chain_cols[l])
        for masters in (True, False):   # W (f32 masters: half a spacing where |w| >= 16, last layer only) and V
            for l, tol in enumerate(sc.weight_bounds(fx, dtype, t.w, t.step, masters)):
                wide = tol != b["w"]
                assert wide.sum() <= (want_w if masters else want_g).get(l, 0) and (tol >= b["w"]).all()
                if l < Lm - 1 and wide.any():
                    assert set(np.flatnonzero(wide.any(axis=0))) <= set(fx.chain_cols[l])
                if l == Lm - 1:
                    assert wide.sum() == (want_w[l] if masters else 0)   # exactly the entries an f32 master cannot hold to the budget
                if l == Lm - 1 and wide.any():
                    assert masters and (np.abs(np_oracle.split(t.w, fx.dims)[l])[wide] >= sc.BIG_W).all()
                    if fx.kind == "shift":
                        assert set(np.flatnonzero(wide.any(axis=1))) <= {sc.UP, sc.UM}


@pytest.mark.parametrize("name", sc.SOFTMAX_SHIFT)
def test_the_recorded_chain_noise_is_the_measured_one(oracle_mod, name):
    fx = sc.fixture(oracle_mod, name)
    for dtype in (sc.F32, sc.BF16):
        seen, now = sc.CHAIN_NOISE_SEEN[name][dtype], max(sc.chain_noise(fx, dtype).values())
        assert abs(now - seen) <= 0.05 * seen + 1e-12, (name, dtype, now, seen)


def test_every_head_has_a_shift_and_a_spread_route():
    """Bookkeeping over the GPU file's route tables (no device): which head a route reaches follows from the plan rules --
    rowblock_kernel.h make_rb_plan and middle4_kernel.h `rowtail` (<= 16 outputs and a last hidden layer <= 128), launch_gemm's
    use_tail (GNN_MLP_TAIL) and output_layer_kernel's register limit of 1024 padded outputs; group_eval.hip launches the full
    head of group_forward_kernel for evaluate_range / ensemble_*_range and the LOSS_ONLY head for train_sampled_observed."""
    from tests import test_saturation_gpu as tg

    def heads(kind):
        out = set()
        for name, dt, env, route in tg.ROUTES:
            row = next(x for x in sc._TABLE if x[0] == name)
            if row[1] != kind or row[3] != sc.SCE:
                continue
            dims = row[2]
            small = dims[-1] <= 16
            if route == "rb":
                out.add("rowblock")
                out.add("tail-bf16" if dt else "middle4-rowtail")      # (what serves propagate / loss / argmax of such a net)
            elif route == "m4":
                out.add("middle4-rowtail" if small and dims[-2] <= 128 else "middle4-register" if small else "middle4-general")
            elif env == tg.GENERIC:
                out.add("tail-bf16" if dt else "tail-f32")
            elif env == tg.NO_TAIL:
                out.add("output-register")
            else:
                out.add("output-three-pass")
        for name, dt in tg.GROUPS:
            if next(x for x in sc._TABLE if x[0] == name)[1] == kind:
                out |= set(tg.GROUP_HEADS)
        return out
    want = {"rowblock", "middle4-rowtail", "middle4-register", "middle4-general", "tail-f32", "tail-bf16", "output-register",
            "output-three-pass", "group-forward-full", "group-forward-loss-only", "rowblock-group"}
    assert heads("shift") == want and heads("spread") == want
