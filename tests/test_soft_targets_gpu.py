"""Every head of the library that reads expected rows, on targets that are not one-hot (fixtures, budgets and the fault models
these comparisons are able to see: tests/soft_target_cases.py, pinned by tests/test_soft_targets_cpu.py).

The expected rows reach the device as dense f32 rows and every output head and evaluation kernel reads them element by
element; the reference sets no condition on them.  Every softmax head has its own copy of the loss expression
sum_j y_j (lse - z_j) and of the delta p - y; on one-hot rows a loss formed as lse - sum y z, a skip by `y > 0` or `y == 1`, the
label column taken for the row, a clamp to [0, 1], targets narrowed to bf16 or a per-row quantity taken from a neighbouring row
are all invisible.  Here row r carries target kind r % 6 (label smoothing, a teacher's softmax, two exact ones, all zero, free
values in [-0.5, 1.5), one-hot), General nets free values on even rows.

A ROUTE is a fixture, a dtype and the environment switches that send it to a head, asserted by the suite's own evidence
(step_launches, rowblock_state, plan_note, specialization, launch counts per kernel class, eval_launches, launches_per_step,
observed_launches) -- the table of tests/test_saturation_gpu.py, and in addition
  784-100-50-10 .................... the prebuilt instances (specialization == 1, rowblock_state == 2), single and group of two
The two "gemm" switches are told apart by the content of plan_note as far as the handle shows it (forced by GNN_MLP_PATH=generic,
or the plan's own refusal for 1100 outputs); that GNN_MLP_TAIL=0 takes output_layer_kernel's register arm instead of tail_kernel is
the host rule plan.hip: use_tail, which no property of a handle reports -- as in tests/test_saturation_gpu.py.

NOT covered: the loss expression of the row-block kernel itself (rowblock_kernel.h, the `if (p.loss)` branch of rowblock_body's
softmax head).  Every caller that reaches the row-block kernel, lone or grouped, asks it for no loss, so no route executes that
copy.  On the "rb" routes the row-block kernel's delta p - y is held through W and V after the steps; the per-row
loss of such a net comes from middle4_kernel's row tail (f32) and from tail_kernel<BF16> (bf16), and those copies are what
calculateLoss / loss_range / evaluate_range compare there.

Against the fp64 oracle (f32; tests/np_oracle.py's matrix form, held to the C oracle here) or np_oracle's *_bf16 (bf16), every
element inside the budget; every comparison prints its worst error as a fraction of its bound.

Measured on an MI355X (91 tests, none skipped, 4.0 s for the file): worst fraction of bound per route, f32 / bf16 -- in f32 it is
W after the steps everywhere, the f32 masters' own rounding, which the float32 restatement of the CPU file shows alike
  row-block (T3, T4, T16 "rb") ......................... 0.014 0.027 0.018 / 2.6e-4 4.0e-4 4.9e-4
  middle4 row tail (T3, T4, T16 ROWBLOCK=0) ............ 0.014 0.027 0.018 / T4 4.0e-4
  middle4 register head (T132), general head (T17, T40)  0.014 0.014 0.014 / 2.9e-4 3.0e-4 2.9e-4
  tail_kernel (T4 generic) ............................. 0.027 / 4.0e-4       output_layer_kernel register arm (TAIL=0) 0.027 / 4.0e-4
  output_layer_kernel three-pass arm (T1100) ........... 0.017 / 2.9e-4
  prebuilt instances (TB, GB) .......................... 0.0046 0.0052 / 7.4e-5 7.4e-5
  General element-wise arms (G4s, G4t, G4i: rb, m4, gemm) 0.024 0.024 0.021 on each route / rb 5.6e-4 5.2e-4 4.5e-4; G17 0.014 / 2.9e-4
  groups (T4, TB, G4s): full head + rowblock_group ..... 0.027 0.0037 0.024 / 5.4e-4 7.4e-5; LOSS_ONLY head 0.024 0.0037 0.026 / 5.3e-4 1.2e-4
  a batch size per member 0.022; train_sampled 0.021 / 4.5e-4; lone observed 5.3e-5 / 6.9e-7; held-out 0.0077 / 0.0016;
  input_gradient 0.0084 / 1.0e-5; gradient_step_indexed 0.024 / 4.9e-4; data-parallel 0.027 / 4.0e-4;
  specialize() (the run-time instances, bit for bit with the unspecialised handle in both dtypes) 0.029 / 2.1e-4 after one step
per-row losses at most 0.004 of their bounds on every route.  No head failed: no kernel was changed."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import input_gradient_cases as igc
from tests import np_oracle
from tests import soft_target_cases as st

pytestmark = pytest.mark.gpu

F32, BF16 = st.F32, st.BF16
GENERIC = {"GNN_MLP_PATH": "generic"}
NO_TAIL = {"GNN_MLP_PATH": "generic", "GNN_MLP_TAIL": "0"}
NO_RB = {"GNN_MLP_ROWBLOCK": "0"}
SWITCHES = ("GNN_MLP_PATH", "GNN_MLP_ROWBLOCK", "GNN_MLP_TAIL", "GNN_MLP_CHAIN", "GNN_MLP_STATIC")
CLASSES = (0, 1, 3, 4)     # GNN_K_FWD_GEMM0, GNN_K_GRAD_GEMM0, GNN_K_MIDDLE, GNN_K_UPDATE (tests/test_launch_counts_gpu.py)

# (fixture, dtype, switches, route): "rb" two launches with the row-block kernel ("rb-prebuilt": its prebuilt instance), "m4" two
# launches with middle4_kernel, "gemm" per-layer GEMMs
ROUTES = []
for _n in ("T3", "T4", "T16"):
    ROUTES += [(_n, F32, {}, "rb"), (_n, BF16, {}, "rb"), (_n, F32, NO_RB, "m4")]                 # row-block; middle4's row tail
ROUTES += [("T4", BF16, NO_RB, "m4")]
ROUTES += [("T4", F32, GENERIC, "gemm"), ("T4", BF16, GENERIC, "gemm"),                          # tail_kernel
           ("T4", F32, NO_TAIL, "gemm"), ("T4", BF16, NO_TAIL, "gemm")]                          # output_layer_kernel's register arm
for _n in ("T132", "T17", "T40"):                                                               # middle4's register / general head
    ROUTES += [(_n, F32, {}, "m4"), (_n, BF16, {}, "m4")]
ROUTES += [("T1100", F32, {}, "gemm"), ("T1100", BF16, {}, "gemm")]                              # the three-pass arm
for _n in ("TB", "GB"):                                                                         # the prebuilt instances
    ROUTES += [(_n, F32, {}, "rb-prebuilt"), (_n, BF16, {}, "rb-prebuilt")]
for _n in ("G4s", "G4t", "G4i"):                                                                # the element-wise arm of each head
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
        if fx.out_kind == st.SCE:
            net = gnn.SoftmaxCrossEntropyNeuralNet(fx.dims, inner_act=fx.inner, dtype=dt, max_batch=fx.rows)
        else:
            net = gnn.GeneralNeuralNet(fx.dims, inner_act=fx.inner, last_act=fx.last, dtype=dt, max_batch=fx.rows)
    evidence = (net.specialization, net.step_launches, net.rowblock_state, net.plan_note)
    if route == "rb-prebuilt":
        assert net.specialization == 1 and net.step_launches == 2 and net.rowblock_state == 2 and net.plan_note == "", evidence
    elif route == "rb":   # no prebuilt instance, and no handle here takes the 16 steps a run-time one needs
        assert net.specialization == 0 and net.step_launches == 2 and net.rowblock_state == 1 and net.plan_note == "", evidence
    elif route == "m4":
        assert net.specialization == 0 and net.step_launches == 2 and net.rowblock_state == 0, evidence
    else:
        assert net.specialization == 0 and net.step_launches == 0 and net.rowblock_state == 0 and net.plan_note != "", evidence
        if "GNN_MLP_PATH" in env:         # forced, and the note says so
            assert "GNN_MLP_PATH=generic" in net.plan_note, evidence
        else:                             # the three-pass arm: more than 1024 padded outputs, which no one-launch kernel takes
            assert (fx.dims[-1] + 15) // 16 * 16 > 1024 and "GNN_MLP_PATH" not in net.plan_note, evidence
    net.set_weights(fx.w)
    assert np.array_equal(net.get_weights(), fx.w)
    return net


def _counts(net):
    return tuple(net.timing_read(c)[1] for c in CLASSES)


class Worst:
    """The worst error of every comparison of a test as a fraction of its bound; each comparison asserts."""

    def __init__(self, what):
        self.what, self.seen = what, {}

    def add(self, key, fraction):
        assert np.isfinite(fraction), (self.what, key)
        self.seen[key] = max(self.seen.get(key, 0.0), float(fraction))
        assert fraction <= 1.0, (self.what, key, fraction)

    def outputs(self, key, fx, dt, p, ref):
        assert np.isfinite(p).all(), (self.what, key)
        self.add(key, np.abs(p - ref).max() / st.out_bound(fx, dt, ref))

    def loss(self, key, fx, dt, loss, ref, terms):
        assert np.isfinite(loss).all(), (self.what, key)
        over = np.abs(loss - ref) / st.loss_bound(fx, dt, terms)
        assert (over <= 1.0).all(), (self.what, key, "row %d" % over.argmax(), "kind %d" % fx.kind[over.argmax()] if len(over) == fx.rows else "", over.max())
        self.add(key, over.max())

    def gradient(self, key, fx, dt, G, ref):
        assert np.isfinite(G).all(), (self.what, key)
        for l, (g, r, b) in enumerate(zip(np_oracle.split(G, fx.dims), np_oracle.split(ref, fx.dims), st.gradient_bounds(fx, dt, ref))):
            over = np.abs(g - r) / b
            assert (over <= 1.0).all(), (self.what, key, "layer %d" % l, over.max(), np.unravel_index(over.argmax(), over.shape))
            self.add(key, over.max())

    def weights(self, key, dt, got, ref, steps=st.N_STEPS):
        assert np.isfinite(got).all(), (self.what, key)
        over = np.abs(got - ref) / st.weight_bound(dt, steps)
        assert (over <= 1.0).all(), (self.what, key, over.max(), int(over.argmax()))
        self.add(key, over.max())

    def report(self):
        print("soft targets, %s: worst fraction of bound %.3g | %s"
              % (self.what, max(self.seen.values()), ", ".join("%s %.3g" % kv for kv in self.seen.items())))


def _flat(per_layer):
    return np.concatenate([per_layer[l].ravel() for l in sorted(per_layer)])


def _hits(what, t, hits, rows=slice(None)):
    lo, hi = t.hits_bounds(rows)
    assert lo <= hits <= hi, (what, hits, lo, hi)


@pytest.mark.parametrize("r", ROUTES, ids=[_route_id(r) for r in ROUTES])
def test_heads_on_soft_targets(gnn, oracle_mod, monkeypatch, r):
    name, dt, env, route = r
    _skip_if_forced(env)
    fx = st.fixture(oracle_mod, name)
    t = fx.truth(dt)
    n, X, Y = fx.rows, fx.X, fx.Y
    if dt == F32:   # the matrix-form truth is the C oracle's
        ref = oracle_mod.OracleNet(fx.dims, out_kind=fx.out_kind, inner_act=fx.inner, last_act=fx.last)
        ref.set_alloc_per_sample(0)
        ref.set_weights(fx.w)
        assert np.allclose(ref.calculate_loss(X, Y), t.loss, rtol=1e-9, atol=1e-9 * t.terms.max())
        ref.close()
    wo = Worst(_route_id(r))
    net = _make(gnn, monkeypatch, fx, dt, env, route)

    # propagate / calculateLoss / calculateWeightGradient on host rows, every element
    wo.outputs("propagate", fx, dt, net.propagate(X), t.out)
    wo.loss("calculateLoss", fx, dt, net.calculateLoss(X, Y), t.loss, t.terms)
    wo.gradient("gradient", fx, dt, _flat(net.calculateWeightGradient(X, Y)), t.G)
    # two steps on host batches: weights and momentum
    for s in range(st.N_STEPS):
        net.gradientStep(X, st.STEP, st.MOMENTUM, False, expected=Y)
    wo.weights("W host", dt, net.get_weights(), t.w)
    wo.weights("V host", dt, net.get_momentum(), t.v)
    net.close()

    # the same on resident rows: loss_range, the hit counts, gradient_step_range + train_range
    res = _make(gnn, monkeypatch, fx, dt, env, route)
    res.upload_dataset(X, Y)
    res.timing_enable(True)
    wo.loss("loss_range", fx, dt, res.loss_range(0, n), t.loss, t.terms)
    _hits("count_hits_range", t, res.count_hits_range(0, n))
    if fx.out_kind == st.SCE:
        hits, loss_sum = res.evaluate_range(0, n)
        _hits("evaluate_range", t, hits)
        wo.add("evaluate_range loss sum", abs(loss_sum - t.loss.sum()) / st.loss_bound(fx, dt, t.terms).sum())
    before = _counts(res)
    res.gradient_step_range(0, n, st.STEP, st.MOMENTUM)
    res.train_range(0, n, st.N_STEPS - 1, st.STEP, st.MOMENTUM)
    if route in ("rb", "m4"):   # per call a chain start; per step a tile launch and a row kernel; no update launch of its own
        assert tuple(a - b for a, b in zip(_counts(res), before)) == (2, st.N_STEPS, st.N_STEPS, 0)
    assert res.time == st.N_STEPS
    wo.weights("W resident", dt, res.get_weights(), t.w)
    wo.weights("V resident", dt, res.get_momentum(), t.v)
    res.close()
    wo.report()


REORDERED = [r for r in ROUTES if r[0] in st.SOFTMAX]


@pytest.mark.parametrize("r", REORDERED, ids=[_route_id(r) for r in REORDERED])
def test_a_row_does_not_depend_on_its_neighbours(gnn, oracle_mod, monkeypatch, r):
    """The rows moved up by one (row 0 last): every 4-row block and 16-row group holds other rows, every row other target kinds
    beside it -- the same bits per row in the loss of resident rows and of host rows."""
    name, dt, env, route = r
    _skip_if_forced(env)
    fx = st.fixture(oracle_mod, name)
    n = fx.rows
    perm = np.r_[1:n, 0]
    assert all(set(perm[g:g + 4]) != set(range(g, min(g + 4, n))) for g in range(0, n, 4))
    got = []
    for order in (np.arange(n), perm):
        net = _make(gnn, monkeypatch, fx, dt, env, route)
        net.upload_dataset(fx.X[order], fx.Y[order])
        got.append((net.loss_range(0, n), net.calculateLoss(fx.X[order], fx.Y[order])))
        net.close()
    for a, b in zip(got[0], got[1]):
        assert np.isfinite(a).all() and np.array_equal(a[perm], b)


GROUPS = [("T4", F32), ("T4", BF16), ("TB", F32), ("TB", BF16), ("G4s", F32)]
OBSERVED_B = 16                                                                      # two draws of 16 from 37 rows: no refill


def _no_switch():
    for k in SWITCHES:
        if k in os.environ:
            pytest.skip("%s forced by the environment" % k)


def _group(gnn, members, dt):
    fx = members[0]
    g = gnn.NetGroup(fx.dims, seeds=[1, 2], out_kind=fx.out_kind, inner_act=fx.inner, last_act=fx.last, dtype=dt, max_batch=fx.rows)
    for k, m in enumerate(members):
        assert m.X is fx.X and m.Y is fx.Y
        g.members[k].set_weights(m.w)
    g.upload_dataset(fx.X, fx.Y)
    assert g.eval_launches == 2 and g.launches_per_step == 2 and g.observed_launches == 3
    if fx.name in ("TB", "GB"):
        assert g.members[0].specialization == 1 and g.members[0].rowblock_state == 2
    return g


def _ensemble_hits_bounds(fx, dt, ts):
    mean = (ts[0].out + ts[1].out) / 2
    srt = np.sort(mean, axis=1)
    safe = (srt[:, -1] - srt[:, -2]) > (2e-3 * np.abs(mean).max() + 1e-3 if dt == BF16 else 1e-3)   # (tests/group_eval_cases.py)
    label = np.array([int(np.flatnonzero(row >= row.max())[-1]) for row in mean])
    sure = int(((label == ts[0].expected) & safe).sum())
    return sure, sure + int((~safe).sum())


@pytest.mark.parametrize("name,dt", GROUPS, ids=["%s-%s" % (n, "bf16" if d else "f32") for n, d in GROUPS])
def test_group_heads_on_soft_targets(gnn, oracle_mod, name, dt):
    _no_switch()
    members = [st.fixture(oracle_mod, name, seed) for seed in (1, 2)]
    fx = members[0]
    ts = [m.truth(dt) for m in members]
    n = fx.rows
    wo = Worst("group %s %s" % (name, "bf16" if dt else "f32"))
    g = _group(gnn, members, dt)
    hits, loss, ens_hits = g.evaluate_range(0, n)                     # the full head: loss and label
    assert g.eval_launches == 2
    lo, hi = _ensemble_hits_bounds(fx, dt, ts)
    assert lo <= ens_hits <= hi, (ens_hits, lo, hi)
    for k, (m, t) in enumerate(zip(members, ts)):
        _hits("member %d" % k, t, hits[k])
        wo.add("member %d loss sum" % k, abs(loss[k] - t.loss.sum()) / st.loss_bound(m, dt, t.terms).sum())
        wo.loss("member %d loss_range" % k, m, dt, g.members[k].loss_range(0, n), t.loss, t.terms)
    # one grouped training call: rowblock_group_kernel, two steps on the one batch of the data set
    g.train_range(0, n, st.N_STEPS, st.STEP, st.MOMENTUM)
    assert g.launches_per_step == 2
    for k, t in enumerate(ts):
        assert g.members[k].time == st.N_STEPS
        wo.weights("member %d W" % k, dt, g.members[k].get_weights(), t.w)
        wo.weights("member %d V" % k, dt, g.members[k].get_momentum(), t.v)
    g.close()
    wo.report()


@pytest.mark.parametrize("name,dt", GROUPS, ids=["%s-%s" % (n, "bf16" if d else "f32") for n, d in GROUPS])
def test_group_validation_head_on_soft_targets(gnn, oracle_mod, name, dt):
    """train_sampled_observed: after every iteration one grouped validation launch, the LOSS_ONLY head of group_forward_kernel,
    over all rows of the data set -- every member's curve value against the mean loss of the oracle stepping on the draws of
    the reference's sampler; the bound is the mean of the per-row budgets."""
    _no_switch()
    members = [st.fixture(oracle_mod, name, seed) for seed in (1, 2)]
    fx = members[0]
    n = fx.rows
    wo = Worst("group validation %s %s" % (name, "bf16" if dt else "f32"))
    g = _group(gnn, members, dt)
    smp = gnn.Sampler(n, seed=1)
    curve = g.train_sampled_observed(smp, 2, OBSERVED_B, st.STEP, st.MOMENTUM, validation_size=n)
    assert g.observed_launches == 3 and curve.shape == (2, 2) and np.isfinite(curve).all()
    for k, m in enumerate(members):
        run = st.sampled_run(oracle_mod, m, dt, 2, OBSERVED_B)
        for i, (w, v) in enumerate(run):
            ref, terms = st.loss_at(m, dt, w, m.X, m.Y)
            wo.add("member %d iteration %d" % (k, i), abs(curve[i, k] - ref.mean()) / st.loss_bound(m, dt, terms).mean())
        wo.weights("member %d W" % k, dt, g.members[k].get_weights(), run[-1][0])
        wo.weights("member %d V" % k, dt, g.members[k].get_momentum(), run[-1][1])
    smp.close()
    g.close()
    wo.report()


def test_group_with_a_batch_size_per_member(gnn, oracle_mod):
    """train_sampled([s0, s1], 2, [8, 16]): the sized twin of the grouped launches; each member against its own oracle run."""
    _no_switch()
    members = [st.fixture(oracle_mod, "T4", seed) for seed in (1, 2)]
    wo = Worst("group sizes T4 f32")
    g = _group(gnn, members, F32)
    smps = [gnn.Sampler(members[0].rows, seed=s) for s in (1, 2)]
    g.train_sampled(smps, 2, [8, 16], st.STEP, st.MOMENTUM)
    assert g.sampled_each_iterations == (2, 0)
    for k, (m, B) in enumerate(zip(members, (8, 16))):
        w, v = st.sampled_run(oracle_mod, m, F32, 2, B, seed=k + 1)[-1]
        wo.weights("member %d W" % k, F32, g.members[k].get_weights(), w)
        wo.weights("member %d V" % k, F32, g.members[k].get_momentum(), v)
    for s in smps:
        s.close()
    g.close()
    wo.report()


# ---- one case each on T4: calls that read Y through code of their own ---------------------------------------------------
BOTH = pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])


def _t4(gnn, oracle_mod, monkeypatch, dt, upload=True):
    fx = st.fixture(oracle_mod, "T4")
    net = _make(gnn, monkeypatch, fx, dt, {}, "rb")
    if upload:
        net.upload_dataset(fx.X, fx.Y)
    return fx, net


@BOTH
def test_train_sampled_reads_soft_rows_through_the_index_vector(gnn, oracle_mod, monkeypatch, dt):
    _no_switch()
    fx, net = _t4(gnn, oracle_mod, monkeypatch, dt, upload=False)
    wo = Worst("train_sampled T4 %s" % ("bf16" if dt else "f32"))
    trainer = gnn.NeuralNetTrainer(fx.X, fx.Y, net, seed=1)
    trainer.train(2, st.STEP, OBSERVED_B, st.MOMENTUM)
    w, v = st.sampled_run(oracle_mod, fx, dt, 2, OBSERVED_B)[-1]
    assert net.time == 2
    wo.weights("W", dt, net.get_weights(), w)
    wo.weights("V", dt, net.get_momentum(), v)
    trainer.sampler.close()
    net.close()
    wo.report()


@BOTH
def test_lone_train_sampled_observed_on_soft_rows(gnn, oracle_mod, monkeypatch, dt):
    _no_switch()
    fx, net = _t4(gnn, oracle_mod, monkeypatch, dt)
    wo = Worst("train_sampled_observed T4 %s" % ("bf16" if dt else "f32"))
    smp = gnn.Sampler(fx.rows, seed=1)
    val = np.empty(2)
    gnn._capi.check(net._lib.gnn_mlp_train_sampled_observed(net._h, smp._h, 2, OBSERVED_B, st.STEP, st.MOMENTUM, 0, fx.rows,
                                                           val.ctypes.data_as(C.POINTER(C.c_double))))
    for i, (w, v) in enumerate(st.sampled_run(oracle_mod, fx, dt, 2, OBSERVED_B)):
        ref, terms = st.loss_at(fx, dt, w, fx.X, fx.Y)
        wo.add("iteration %d" % i, abs(val[i] - ref.mean()) / st.loss_bound(fx, dt, terms).mean())
    smp.close()
    net.close()
    wo.report()


@BOTH
def test_held_out_loss_curve_on_soft_rows(gnn, oracle_mod, monkeypatch, dt):
    """train_sampled_held_out(rule="loss"): the held-out rows carry the six target kinds; every point's loss sum against the
    oracle inside the summed per-row budgets, the best point the oracle's (decided by more than twice the budgets of both points:
    tests/test_soft_targets_cpu.py), the weights kept there the oracle's at that iteration."""
    _no_switch()
    fx, net = _t4(gnn, oracle_mod, monkeypatch, dt)
    wo = Worst("held-out T4 %s" % ("bf16" if dt else "f32"))
    net.upload_held_out(fx.Xh, fx.Yh)
    h = st.HELD
    smp = gnn.Sampler(fx.rows, seed=1)
    hits, loss, best, w_best = net.train_sampled_held_out(smp, h["iterations"], h["batch"], h["step"], st.MOMENTUM, h["every"], rule="loss")
    ref_loss, bound, ref_hits = st.held_out_curve(oracle_mod, fx, dt)
    assert len(loss) == len(ref_loss) == 3
    for p in range(3):
        wo.add("point %d" % p, abs(loss[p] - ref_loss[p]) / bound[p])
        assert ref_hits[p][0] <= hits[p] <= ref_hits[p][1], (p, hits[p], ref_hits[p])
    assert best == int(ref_loss.argmin()) == gnn.best_point(hits, loss, "loss")
    at = (best + 1) * h["every"]
    wo.weights("best weights", dt, w_best, st.sampled_run(oracle_mod, fx, dt, at, h["batch"], step=h["step"])[-1][0], steps=at)
    smp.close()
    net.close()
    wo.report()


@BOTH
def test_input_gradient_on_soft_rows(gnn, oracle_mod, monkeypatch, dt):
    _no_switch()
    fx, net = _t4(gnn, oracle_mod, monkeypatch, dt, upload=False)
    fn = igc.input_gradient_bf16 if dt else igc.input_gradient
    ref = fn(fx.Ws, fx.X, fx.Y, fx.inner, fx.out_kind, fx.last)
    err, budget = igc.within(net.input_gradient(fx.X, fx.Y), ref, bf16=bool(dt))
    print("soft targets, input_gradient T4 %s: %.3g of its bound" % ("bf16" if dt else "f32", err / budget))
    assert err <= budget
    net.upload_dataset(fx.X, fx.Y)
    err, budget = igc.within(net.input_gradient_range(0, fx.rows), ref, bf16=bool(dt))
    print("soft targets, input_gradient_range T4 %s: %.3g of its bound" % ("bf16" if dt else "f32", err / budget))
    assert err <= budget
    net.close()


INDEXED = [[35, 2, 8, 3, 4, 18, 12, 9, 26, 33, 1], [0, 36, 7, 16, 22, 29, 32, 21, 5]]   # two batches of odd length, every kind in each


@BOTH
def test_gradient_step_indexed_on_soft_rows(gnn, oracle_mod, monkeypatch, dt):
    _no_switch()
    fx, net = _t4(gnn, oracle_mod, monkeypatch, dt)
    wo = Worst("gradient_step_indexed T4 %s" % ("bf16" if dt else "f32"))
    w, v = fx.w.copy(), np.zeros_like(fx.w)
    for idx in INDEXED:
        assert set(fx.kind[idx]) == set(range(st.N_KINDS))
        net.gradient_step_indexed(idx, st.STEP, st.MOMENTUM)
        w, v = st.oracle_step(fx, dt, w, v, fx.X[idx], fx.Y[idx])
    wo.weights("W", dt, net.get_weights(), w)
    wo.weights("V", dt, net.get_momentum(), v)
    net.close()
    wo.report()


@BOTH
def test_data_parallel_step_on_soft_rows(gnn, oracle_mod, dt):
    """Two replicas on device 0, one reducer: W and V against the whole-batch oracle (2e-6 per step; bf16 2e-4)."""
    _no_switch()
    fx = st.fixture(oracle_mod, "T4")
    t = fx.truth(dt)
    wo = Worst("data-parallel T4 %s" % ("bf16" if dt else "f32"))
    net = gnn.DataParallelNeuralNet(fx.dims, devices=[0, 0], inner_act=fx.inner, dtype=dt, max_batch=fx.rows, reducer=gnn.REDUCE_DIRECT)
    net.set_weights(fx.w)
    net.upload_dataset(fx.X, fx.Y)
    net.train_range(0, fx.rows, st.N_STEPS, st.STEP, st.MOMENTUM)
    net.synchronize()
    assert net.time == st.N_STEPS and net.replicas_identical()
    wo.weights("W", dt, net.get_weights(), t.w)
    wo.weights("V", dt, net.get_momentum(), t.v)
    net.close()
    wo.report()


@BOTH
def test_the_specialised_handle_agrees_bit_for_bit_on_soft_rows(gnn, oracle_mod, monkeypatch, dt):
    """net.specialize(): the kernels instantiated at run time for this shape (f32 and bf16 alike: the row-block kernel and
    middle4_kernel's training instance), which no other handle of this file reaches -- none takes the 16 steps after which a
    handle instantiates them by itself.  loss_range and one step, bit for bit with the unspecialised handle, and against the
    oracle so that two handles wrong alike do not pass."""
    _no_switch()
    fx, a = _t4(gnn, oracle_mod, monkeypatch, dt)
    _, b = _t4(gnn, oracle_mod, monkeypatch, dt)
    t = fx.truth(dt)
    wo = Worst("specialize T4 %s" % ("bf16" if dt else "f32"))
    assert b.specialize() == 2 and b.rowblock_state == 3, "run-time instantiation failed (hiprtc unavailable?)"
    assert a.specialization == 0 and a.rowblock_state == 1
    loss = b.loss_range(0, fx.rows)
    assert np.array_equal(a.loss_range(0, fx.rows), loss)
    wo.loss("loss_range", fx, dt, loss, t.loss, t.terms)
    a.gradient_step_range(0, fx.rows, st.STEP, st.MOMENTUM)
    b.gradient_step_range(0, fx.rows, st.STEP, st.MOMENTUM)
    assert b.specialization == 2 and b.rowblock_state == 3 and a.rowblock_state == 1
    assert np.array_equal(a.get_weights(), b.get_weights()) and np.array_equal(a.get_momentum(), b.get_momentum())
    w, v = st.oracle_step(fx, dt, fx.w.copy(), np.zeros_like(fx.w), fx.X, fx.Y)
    wo.weights("W", dt, b.get_weights(), w, steps=1)
    wo.weights("V", dt, b.get_momentum(), v, steps=1)
    a.close()
    b.close()
    wo.report()


@BOTH
def test_the_expected_class_of_soft_rows(gnn, oracle_mod, monkeypatch, dt):
    """confusion_range: row e counts the rows whose expected class (the LAST exact 1.0, else class 0: MT:186-188) is e -- for
    a lone net, the members of a group and the ensemble."""
    _no_switch()
    members = [st.fixture(oracle_mod, "T4", seed) for seed in (1, 2)]
    fx = members[0]
    d = fx.dims[-1]
    want = np.bincount(st.expected_class(fx.Y), minlength=d)
    assert not np.array_equal(want, np.bincount(fx.Y.argmax(axis=1), minlength=d))     # (the argmax of the row counts otherwise)
    _, net = _t4(gnn, oracle_mod, monkeypatch, dt)
    conf = net.confusion_range(0, fx.rows)
    assert np.array_equal(conf.sum(axis=1), want)
    _hits("lone net", fx.truth(dt), int(np.trace(conf)))
    net.close()
    g = _group(gnn, members, dt)
    member, ens = g.confusion_range(0, fx.rows)
    for k, m in enumerate(members):
        assert np.array_equal(member[k].sum(axis=1), want), "member %d" % k
        _hits("member %d" % k, m.truth(dt), int(np.trace(member[k])))
    assert np.array_equal(ens.sum(axis=1), want)
    lo, hi = _ensemble_hits_bounds(fx, dt, [m.truth(dt) for m in members])
    assert lo <= int(np.trace(ens)) <= hi
    g.close()
