"""Every output head of the library on saturated logits in mixed-regime batches (fixtures, budgets and the fault models these
comparisons are able to see: tests/saturation_cases.py, pinned by tests/test_saturation_cpu.py).

Every softmax head subtracts the row maximum before __expf and forms the loss as lse - z.  With every logit within +-80 any
finite "maximum" does; here rows of all-high (+150), all-low (-150) and neutral logits share each 4-row block and each 16-lane
row, or the logits of one row spread over +-300 -- a maximum taken over the wrong lanes, over a padding column, left stale or at 0,
no subtraction, or a loss formed as -log p returns NaN, inf or a wrong number on these rows.

A ROUTE is a fixture, a dtype and the environment switches that send it to a head; the route assertions are the suite's
(step_launches, rowblock_state, plan_note, launch counts per kernel class, eval_launches, launches_per_step):
  two-launch, row-block kernel ....... rowblock_body's head (no-label arm: every gradient and step; the library never asks this
                                       kernel for probabilities, losses or labels -- on an f32 net those come from middle4_kernel's
                                       forward-only instance, on a bf16 net from the per-layer GEMMs + tail_kernel<BF16>)
  GNN_MLP_ROWBLOCK=0 ................. middle4_kernel's row tail (<= 16 outputs, last hidden layer <= 128)
  last hidden layer of 132 ........... middle4_kernel's register head (<= 16 outputs, no row tail, no row-block kernel)
  17 / 40 outputs .................... middle4_kernel's general head
  GNN_MLP_PATH=generic ............... tail_kernel f32 / bf16; with GNN_MLP_TAIL=0 output_layer_kernel's register arm
  1100 outputs ....................... output_layer_kernel's three-pass arm
  NetGroup ........................... group_forward_kernel's full head (evaluate_range and ensemble_*_range: eval_launches 2),
                                       its LOSS_ONLY head (the validation pass of train_sampled_observed: observed_launches
                                       3), rowblock_group_kernel (train_range: launches_per_step 2)
propagate returns the caller's rows only: that padding rows hold no NaN cannot be seen through the interface and is not checked.
Against the fp64 oracle (f32; tests/np_oracle.py's matrix form, held to the C oracle here) or np_oracle's *_bf16 (bf16).

Tried once on an MI355X: with rowblock_body's no-label maximum taken over all four columns of a lane (the padding columns' exact
0 included) the 357 tests of test_parity / chain_shapes / random_shapes / bf16 / group / static_instances _gpu.py passed, and here
the eight routes through that head with padding columns (S3, S4, S4s "rb" in f32 and bf16, the S4 groups) failed."""
import os

import numpy as np
import pytest

from tests import np_oracle
from tests import saturation_cases as sc

pytestmark = pytest.mark.gpu

F32, BF16 = sc.F32, sc.BF16
GENERIC = {"GNN_MLP_PATH": "generic"}
NO_TAIL = {"GNN_MLP_PATH": "generic", "GNN_MLP_TAIL": "0"}
NO_RB = {"GNN_MLP_ROWBLOCK": "0"}
SWITCHES = ("GNN_MLP_PATH", "GNN_MLP_ROWBLOCK", "GNN_MLP_TAIL", "GNN_MLP_CHAIN", "GNN_MLP_STATIC")
CLASSES = (0, 1, 3, 4)     # GNN_K_FWD_GEMM0, GNN_K_GRAD_GEMM0, GNN_K_MIDDLE, GNN_K_UPDATE (tests/test_launch_counts_gpu.py)

# (fixture, dtype, switches, route): "rb" two launches with the row-block kernel, "m4" two launches with middle4_kernel,
# "gemm" per-layer GEMMs
ROUTES = []
for _n in ("S3", "S4", "S4s", "S16", "P4", "P16"):
    ROUTES += [(_n, F32, {}, "rb"), (_n, BF16, {}, "rb")]
for _n in ("S3", "S4", "S4s", "S16", "P4", "P16"):                       # middle4's row tail
    ROUTES += [(_n, F32, NO_RB, "m4")]
ROUTES += [("S4", BF16, NO_RB, "m4"), ("P4", BF16, NO_RB, "m4")]
for _n in ("S132", "P132", "S17", "S40", "P17"):                         # middle4's register head / general head
    ROUTES += [(_n, F32, {}, "m4"), (_n, BF16, {}, "m4")]
for _n in ("S4", "P4"):                                                  # tail_kernel; output_layer_kernel's register arm
    ROUTES += [(_n, F32, GENERIC, "gemm"), (_n, BF16, GENERIC, "gemm"), (_n, F32, NO_TAIL, "gemm"), (_n, BF16, NO_TAIL, "gemm")]
for _n in ("S1100", "P1100"):                                            # output_layer_kernel's three-pass arm
    ROUTES += [(_n, F32, {}, "gemm"), (_n, BF16, {}, "gemm")]
for _n in ("G_ident", "G_leaky", "G_relu", "G_sigm", "G_tanh"):          # GeneralNeuralNet: the element-wise arm of each head
    ROUTES += [(_n, F32, {}, "rb"), (_n, F32, NO_RB, "m4"), (_n, F32, GENERIC, "gemm"), (_n, BF16, {}, "rb")]
ROUTES += [("G17", F32, {}, "m4"), ("G17", BF16, GENERIC, "gemm")]


def _route_id(r):
    name, dt, env, route = r
    sw = "".join("-" + k[len("GNN_MLP_"):].lower() + v for k, v in sorted(env.items()))
    return "%s-%s-%s%s" % (name, "bf16" if dt else "f32", route, sw)


def _skip_if_forced(env):
    for k in SWITCHES:
        if k in os.environ and os.environ[k] != env.get(k):
            pytest.skip("%s forced by the environment" % k)


def _make(gnn, monkeypatch, fx, dt, env, route):
    with monkeypatch.context() as m:
        for k, v in env.items():
            m.setenv(k, v)
        if fx.out_kind == sc.SCE:
            net = gnn.SoftmaxCrossEntropyNeuralNet(fx.dims, inner_act=fx.inner, dtype=dt, max_batch=fx.rows)
        else:
            net = gnn.GeneralNeuralNet(fx.dims, inner_act=fx.inner, last_act=fx.last, dtype=dt, max_batch=fx.rows)
    # the route; none of these shapes has a prebuilt instance and no handle here takes the 16 steps a run-time one needs
    assert net.specialization == 0
    if route == "rb":
        assert net.step_launches == 2 and net.rowblock_state >= 1, (net.step_launches, net.rowblock_state, net.plan_note)
        assert net.plan_note == ""
    elif route == "m4":
        assert net.step_launches == 2 and net.rowblock_state == 0, (net.step_launches, net.rowblock_state, net.plan_note)
    else:
        assert net.step_launches == 0 and net.rowblock_state == 0 and net.plan_note != "", (net.step_launches, net.plan_note)
        if "GNN_MLP_PATH" not in env:     # the three-pass arm: more than 1024 padded outputs, which no one-launch kernel takes
            assert (fx.dims[-1] + 15) // 16 * 16 > 1024
    net.set_weights(fx.w)
    assert np.array_equal(net.get_weights(), fx.w)
    return net


def _counts(net):
    return tuple(net.timing_read(c)[1] for c in CLASSES)


def _out_bounds(fx, dt, t):
    """(outputs, loss): the softmax budgets; GeneralNeuralNet: the suite's 2e-5 / 1e-4 rel + 1e-5 (bf16: the bf16 budgets), the
    output bound times max |out| where the last activation is unbounded (the losses there are 1e4 and more: their bound is the
    relative term, the absolute one is kept for the neutral rows)."""
    b = sc.BUDGET[dt]
    if fx.out_kind == sc.SCE:
        return b["p"], b["l_rel"] * np.abs(t.loss) + b["l_abs"]
    unbounded = fx.last in (sc.IDENT, sc.LEAKY, sc.RELU)
    p, rel, ab = (b["p"], b["l_rel"], b["l_abs"]) if dt == BF16 else (2e-5, 1e-4, 1e-5)
    return p * (np.abs(t.out).max() if unbounded else 1.0), rel * np.abs(t.loss) + ab


def _assert_outputs(what, fx, dt, t, p, loss):
    pb, lb = _out_bounds(fx, dt, t)
    assert np.isfinite(p).all() and np.isfinite(loss).all(), what
    ep, el = np.abs(p - t.out).max(), (np.abs(loss - t.loss) / lb).max()
    print("%s: output error %.3g (bound %.3g), loss error %.3g of its bound" % (what, ep, pb, el))
    assert ep <= pb, what
    assert el <= 1.0, what


def _assert_elementwise(what, got, ref, bounds, dims):
    assert np.isfinite(got).all(), what
    worst = 0.0
    for l, (g, r) in enumerate(zip(np_oracle.split(got, dims), np_oracle.split(ref, dims))):
        over = np.abs(g - r) / bounds[l]
        worst = max(worst, over.max())
        assert (over <= 1.0).all(), (what, "layer %d" % l, over.max(), np.unravel_index(over.argmax(), over.shape))
    print("%s: %.3g of its bound" % (what, worst))


def _flat(per_layer):
    return np.concatenate([per_layer[l].ravel() for l in sorted(per_layer)])


@pytest.mark.parametrize("r", ROUTES, ids=[_route_id(r) for r in ROUTES])
def test_heads_on_saturated_rows(gnn, oracle_mod, monkeypatch, r):
    name, dt, env, route = r
    _skip_if_forced(env)
    fx = sc.fixture(oracle_mod, name)
    t = fx.truth(dt)
    n, X, Y = fx.rows, fx.X, fx.Y
    if dt == F32:   # the matrix-form truth is the C oracle's
        ref = oracle_mod.OracleNet(fx.dims, out_kind=fx.out_kind, inner_act=fx.inner, last_act=fx.last)
        ref.set_alloc_per_sample(0)
        ref.set_weights(fx.w)
        assert np.abs(ref.propagate(X) - t.out).max() <= 1e-9 * max(1.0, np.abs(t.out).max())
        assert np.allclose(ref.calculate_loss(X, Y), t.loss, rtol=1e-9, atol=1e-12)
        ref.close()
    net = _make(gnn, monkeypatch, fx, dt, env, route)

    # propagate / calculateLoss / argmax on host rows
    _assert_outputs("host rows", fx, dt, t, net.propagate(X), net.calculateLoss(X, Y))
    lab = net.argmax(X)
    assert np.array_equal(lab[t.safe], t.label[t.safe]), (lab, t.label, t.safe)
    # calculateWeightGradient, every element
    _assert_elementwise("gradient", _flat(net.calculateWeightGradient(X, Y)), t.G, sc.gradient_bounds(fx, dt, t.G), fx.dims)
    # two steps on host batches: weights and momentum
    wb, vb = sc.weight_bounds(fx, dt, t.w, t.step), sc.weight_bounds(fx, dt, t.w, t.step, masters=False)
    for s in range(sc.N_STEPS):
        net.gradientStep(X, t.step, sc.MOMENTUM, False, expected=Y)
    _assert_elementwise("W after host steps", net.get_weights(), t.w, wb, fx.dims)
    _assert_elementwise("V after host steps", net.get_momentum(), t.v, vb, fx.dims)
    net.close()

    # the same on resident rows: loss_range / argmax_range, gradient_step_range + train_range (the no-label arm)
    res = _make(gnn, monkeypatch, fx, dt, env, route)
    res.upload_dataset(X, Y)
    res.timing_enable(True)
    loss = res.loss_range(0, n)
    assert np.isfinite(loss).all() and (np.abs(loss - t.loss) <= _out_bounds(fx, dt, t)[1]).all()
    assert np.array_equal(res.argmax_range(0, n)[t.safe], t.label[t.safe])
    before = _counts(res)
    res.gradient_step_range(0, n, t.step, sc.MOMENTUM)
    res.train_range(0, n, sc.N_STEPS - 1, t.step, sc.MOMENTUM)
    if route in ("rb", "m4"):   # per call a chain start; per step a tile launch and a row kernel; no update launch of its own
        assert tuple(a - b for a, b in zip(_counts(res), before)) == (2, sc.N_STEPS, sc.N_STEPS, 0)
    assert res.time == sc.N_STEPS
    _assert_elementwise("W after resident steps", res.get_weights(), t.w, wb, fx.dims)
    _assert_elementwise("V after resident steps", res.get_momentum(), t.v, vb, fx.dims)
    res.close()


REORDERED = [r for r in ROUTES if r[0] in sc.SOFTMAX_SHIFT]


@pytest.mark.parametrize("r", REORDERED, ids=[_route_id(r) for r in REORDERED])
def test_a_row_does_not_depend_on_its_neighbours(gnn, oracle_mod, monkeypatch, r):
    """The rows moved up by one (row 0 last): every 4-row block and 16-row group holds other rows, every high row other
    neighbours -- the same bits per row in the probabilities and in the loss of resident rows."""
    name, dt, env, route = r
    _skip_if_forced(env)
    fx = sc.fixture(oracle_mod, name)
    n = fx.rows
    perm = np.r_[1:n, 0]
    assert all(set(perm[g:g + 4]) != set(range(g, min(g + 4, n))) for g in range(0, n, 4))
    got = []
    for order in (np.arange(n), perm):
        net = _make(gnn, monkeypatch, fx, dt, env, route)
        net.upload_dataset(fx.X[order], fx.Y[order])
        got.append((net.propagate(fx.X[order]), net.loss_range(0, n), net.calculateLoss(fx.X[order], fx.Y[order])))
        net.close()
    for a, b in zip(got[0], got[1]):
        assert np.isfinite(a).all() and np.array_equal(a[perm], b)


GROUPS = [("S4", F32), ("S4", BF16), ("P4", F32), ("P4", BF16)]
GROUP_HEADS = ("group-forward-full", "group-forward-loss-only", "rowblock-group")   # what each group case reaches, in this order
OBSERVED_B = 16                                                                      # two draws of 16 from 37 rows: no refill


def _group(gnn, members, dt, order=None):
    fx = members[0]
    order = np.arange(fx.rows) if order is None else order
    g = gnn.NetGroup(fx.dims, seeds=[1, 2], inner_act=fx.inner, dtype=dt, max_batch=fx.rows)
    for k, m in enumerate(members):
        assert np.array_equal(m.X, fx.X) and np.array_equal(m.Y, fx.Y)
        g.members[k].set_weights(m.w)
    g.upload_dataset(fx.X[order], fx.Y[order])
    return g


@pytest.mark.parametrize("name,dt", GROUPS, ids=["%s-%s" % (n, "bf16" if d else "f32") for n, d in GROUPS])
def test_group_heads_on_saturated_rows(gnn, oracle_mod, name, dt):
    for k in SWITCHES:
        if k in os.environ:
            pytest.skip("%s forced by the environment" % k)
    members = [sc.fixture(oracle_mod, name, seed) for seed in (1, 2)]
    fx, b = members[0], sc.BUDGET[dt]
    ts = [m.truth(dt) for m in members]
    n, X, Y = fx.rows, fx.X, fx.Y
    g = _group(gnn, members, dt)
    assert g.eval_launches == 2 and g.launches_per_step == 2
    expected = Y.argmax(axis=1)
    hits, loss, ens_hits = g.evaluate_range(0, n)                     # the full head: loss and label
    mean = g.ensemble_propagate_range(0, n)                           # the full head: probabilities of resident rows
    lab = g.ensemble_argmax_range(0, n)
    assert g.eval_launches == 2
    mean_t = (ts[0].out + ts[1].out) / 2
    assert np.isfinite(mean).all() and np.isfinite(loss).all()
    print(name, "mean-output error", np.abs(mean - mean_t).max(), "hits", hits.tolist(), "ensemble hits", ens_hits)
    assert np.abs(mean - mean_t).max() <= b["p"]
    srt = np.sort(mean_t, axis=1)
    ens_safe = (srt[:, -1] - srt[:, -2]) > (2e-3 * np.abs(mean_t).max() + 1e-3 if dt == BF16 else 1e-3)
    ens_label = np.array([int(np.flatnonzero(row >= row.max())[-1]) for row in mean_t])
    assert np.array_equal(lab[ens_safe], ens_label[ens_safe])
    sure = int(((ens_label == expected) & ens_safe).sum())
    assert sure <= ens_hits <= sure + int((~ens_safe).sum())
    for k, t in enumerate(ts):
        sure = int(((t.label == expected) & t.safe).sum())             # (Truth.hits_bounds of tests/group_eval_cases.py)
        assert sure <= hits[k] <= sure + int((~t.safe).sum()), "member %d" % k
        print("  member", k, "loss sum", loss[k], "oracle", t.loss.sum())
        assert abs(loss[k] - t.loss.sum()) <= (b["l_rel"] * np.abs(t.loss) + b["l_abs"]).sum(), "member %d" % k
        own = g.members[k].loss_range(0, n)                            # ... and per row through the member's own handle
        assert (np.abs(own - t.loss) <= b["l_rel"] * np.abs(t.loss) + b["l_abs"]).all(), "member %d" % k
    if fx.kind == "shift":   # resident probabilities do not depend on a row's neighbours: the rows moved up by one, the same bits
        perm = np.r_[1:n, 0]
        gp = _group(gnn, members, dt, perm)
        assert np.array_equal(gp.ensemble_propagate_range(0, n), mean[perm])
        gp.close()
    # one grouped training call: rowblock_group_kernel, two steps on the one batch of the data set
    g.train_range(0, n, sc.N_STEPS, sc.STEP, sc.MOMENTUM)
    assert g.launches_per_step == 2
    for k, (m, t) in enumerate(zip(members, ts)):
        wb, vb = sc.weight_bounds(m, dt, t.w, t.step), sc.weight_bounds(m, dt, t.w, t.step, masters=False)
        assert g.members[k].time == sc.N_STEPS
        _assert_elementwise("member %d W" % k, g.members[k].get_weights(), t.w, wb, m.dims)
        _assert_elementwise("member %d V" % k, g.members[k].get_momentum(), t.v, vb, m.dims)
    g.close()


@pytest.mark.parametrize("name,dt", GROUPS, ids=["%s-%s" % (n, "bf16" if d else "f32") for n, d in GROUPS])
def test_group_validation_head_on_saturated_rows(gnn, oracle_mod, name, dt):
    """train_sampled_observed: after every iteration one grouped validation launch, the LOSS_ONLY head of group_forward_kernel
    (its own maximum, its own __expf sum, its own lse - z), over all rows of the data set -- every member's curve value against
    the oracle's mean loss.  First one iteration with a step of 2^-40 (a step must be positive; this one moves no weight by
    more than 1e-9): the mean loss of the fixture's own weights.  Then two iterations with the suite's step on the draws of
    the reference's sampler: the oracle stepping on the same rows."""
    for k in SWITCHES:
        if k in os.environ:
            pytest.skip("%s forced by the environment" % k)
    members = [sc.fixture(oracle_mod, name, seed) for seed in (1, 2)]
    fx, b = members[0], sc.BUDGET[dt]
    n, B = fx.rows, OBSERVED_B

    def bound(loss):
        return (b["l_rel"] * np.abs(loss) + b["l_abs"]).mean()

    g = _group(gnn, members, dt)
    assert g.launches_per_step == 2 and g.observed_launches == 3 and g.eval_launches == 2
    smp = gnn.Sampler(n, seed=1)
    curve = g.train_sampled_observed(smp, 1, B, 2.0 ** -40, 0.0, validation_size=n)
    assert curve.shape == (1, 2) and np.isfinite(curve).all()
    for k, m in enumerate(members):
        assert np.abs(g.members[k].get_weights() - m.w).max() <= 1e-9, "member %d" % k
        ref = m.truth(dt).loss
        print(name, "member", k, "mean loss", curve[0, k], "oracle", ref.mean(), "bound", bound(ref))
        assert abs(curve[0, k] - ref.mean()) <= bound(ref), "member %d" % k
    smp.close()
    g.close()

    g = _group(gnn, members, dt)
    smp, ref_smp = gnn.Sampler(n, seed=1), oracle_mod.Sampler(n, seed=1)
    curve = g.train_sampled_observed(smp, 2, B, sc.STEP, sc.MOMENTUM, validation_size=n)
    assert g.observed_launches == 3 and curve.shape == (2, 2) and np.isfinite(curve).all()
    draws = [ref_smp.sample(B) for _ in range(2)]
    assert all(len(d) == B for d in draws)
    for k, m in enumerate(members):
        w, v = m.w.copy(), np.zeros_like(m.w)
        for i, idx in enumerate(draws):
            w, v = sc.oracle_step(m, dt, w, v, idx, sc.STEP)
            ref = sc.loss_at(m, dt, w)
            print(name, "member", k, "iteration", i, "mean loss", curve[i, k], "oracle", ref.mean(), "bound", bound(ref))
            assert abs(curve[i, k] - ref.mean()) <= bound(ref), "member %d, iteration %d" % (k, i)
    smp.close()
    g.close()
