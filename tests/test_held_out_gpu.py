"""The held-out set on the GPU: the evaluation passes on either resident set (gnn_mlp_*_set_range), the independence of the two
sets, and the training loops that record the held-out curve and keep the best weights on the device
(gnn_mlp_train_sampled_held_out, gnn_mlp_group_train_sampled_held_out; csrc/keep_best_kernel.h).

Bitwise comparisons are against a TWIN: a net or group with the same weights that reaches the same state through the calls that
existed before -- its training set holding the rows, its training cut into one call per interval with evaluate_range and
get_weights behind each.  Against the fp64 oracle only what tests/test_held_out_cpu.py shows an f32 run cannot blur is asserted:
the loss rule's point on T1 / T3 and the loss curve inside the budget of test_group_eval_gpu.py (2e-4 relative + 2e-4 per row),
the hits at every point and the hits rule's point on T1h / T2h."""
import ctypes as C

import numpy as np
import pytest

from tests import group_eval_cases as gc
from tests import held_out_cases as hc
from tests.test_group_eval_gpu import _check_against

pytestmark = pytest.mark.gpu


# ---- G1: evaluation on the held-out set ------------------------------------------------------------------------------------------
def _other_rows(case, n=40):
    rng = np.random.default_rng(99)
    return rng.standard_normal((n, case.dims[0])), np.eye(case.dims[-1])[rng.integers(0, case.dims[-1], n)]


def _eval_group(gnn, case, weights, max_batch=1024):
    g = gnn.NetGroup(case.dims, list(range(1, case.K + 1)), out_kind=case.kind, inner_act=case.inner, last_act=case.last,
                     dtype=case.dtype, max_batch=max_batch)
    for k in range(case.K):
        g.members[k].set_weights(weights[k])
    return g


class _HeldMember:
    def __init__(self, member, twin_member):
        self.m, self.t = member, twin_member

    def count_hits_range(self, first, n):
        return self.m.count_hits_range(first, n, held_out=True)

    def loss_range(self, first, n):  # (the member's own per-row losses of these rows: the twin holds them as its training set)
        return self.t.loss_range(first, n)


class _HeldView:
    """The group's held-out calls under the names test_group_eval_gpu._check_against uses."""

    def __init__(self, g, twin):
        self.g = g
        self.members = [_HeldMember(m, t) for m, t in zip(g.members, twin.members)]

    def evaluate_range(self, first, n):
        return self.g.evaluate_range(first, n, held_out=True)

    def ensemble_propagate_range(self, first, n):
        return self.g.ensemble_propagate_range(first, n, held_out=True)

    def ensemble_argmax_range(self, first, n):
        return self.g.ensemble_argmax_range(first, n, held_out=True)


@pytest.mark.parametrize("name", ["E1", "E1b", "E2", "E4", "E6c", "E7", "E7b"])
def test_group_evaluation_on_the_held_out_set(gnn, oracle_mod, name):
    case, t = gc.CASES[name], gc.truth(oracle_mod, name)
    w = [gc.member_weights(oracle_mod, case, k) for k in range(case.K)]
    n = case.rows
    twin = _eval_group(gnn, case, w)
    twin.upload_dataset(gc.inputs(case), t.Y)
    g = _eval_group(gnn, case, w)
    g.upload_dataset(*_other_rows(case))
    g.upload_held_out(gc.inputs(case), t.Y)
    assert g.held_out_size == n and all(m.held_out_size == n for m in g.members) and g.members[0].dataset_size == 40
    assert g.eval_launches == (2 if case.grouped else 0)
    for a, b in zip(g.evaluate_range(0, n, held_out=True), twin.evaluate_range(0, n)):
        assert np.array_equal(a, b)
    for a, b in zip(g.evaluate_range(held_out=True), twin.evaluate_range()):  # (n=None: the rest of the named set)
        assert np.array_equal(a, b)
    assert np.array_equal(g.ensemble_propagate_range(0, n, held_out=True), twin.ensemble_propagate_range(0, n))
    assert np.array_equal(g.ensemble_argmax_range(3, n - 7, held_out=True), twin.ensemble_argmax_range(3, n - 7))
    for a, b in zip(g.confusion_range(0, n, labels=True, held_out=True), twin.confusion_range(0, n, labels=True)):
        assert np.array_equal(a, b)
    for m, tm in zip(g.members, twin.members):
        assert m.evaluate_range(0, n, held_out=True) == tm.evaluate_range(0, n)
        assert np.array_equal(m.confusion_range(0, n, held_out=True), tm.confusion_range(0, n))
        assert np.array_equal(m.labels_range(5, n - 5, held_out=True), tm.labels_range(5, n - 5))
        assert m.count_hits_range(0, n, held_out=True) == tm.count_hits_range(0, n)
        assert gnn.accuracy(m, held_out=True) == gnn.accuracy(tm)
    # held_out=False is the call without the keyword: the training set, untouched by the held-out upload
    for a, b in zip(g.evaluate_range(0, 40, held_out=False), g.evaluate_range(0, 40)):
        assert np.array_equal(a, b)
    assert np.array_equal(g.ensemble_propagate_range(0, 40, held_out=False), g.ensemble_propagate_range(0, 40))
    for a, b in zip(g.confusion_range(0, 40, held_out=False), g.confusion_range(0, 40)):
        assert np.array_equal(a, b)
    assert g.members[0].evaluate_range(0, 40, held_out=False) == g.members[0].evaluate_range(0, 40)
    # inside the oracle's bounds exactly as test_group_eval_gpu states them
    _check_against(_HeldView(g, twin), case, t, case.K)
    g.close()
    twin.close()


def _lone(gnn, case, w, max_batch=1024):
    net = gnn.NeuralNet(case.dims, case.kind, case.inner, case.last, gnn.LOSS_HALF_SQUARED, seed=1, dtype=case.dtype, max_batch=max_batch)
    net.set_weights(w)
    return net


@pytest.mark.parametrize("name, env, max_batch", [("E1", {}, 1024), ("E1b", {}, 1024), ("E4", {}, 1024), ("E1b", {}, 64),
                                                  ("E1", {"GNN_MLP_PATH": "generic"}, 1024), ("E1", {"GNN_MLP_EVAL_ROWS": "64"}, 32)])
def test_lone_evaluation_on_the_held_out_set(gnn, oracle_mod, monkeypatch, name, env, max_batch):
    """(E1b at max_batch 64, E1 with evaluation blocks of 64 rows: the 150 rows make three blocks.)"""
    case, t = gc.CASES[name], gc.truth(oracle_mod, name)
    for k, v in env.items():
        monkeypatch.setenv(k, v)  # (read once, at create)
    w, n = gc.member_weights(oracle_mod, case, 0), case.rows
    twin = _lone(gnn, case, w, max_batch)
    twin.upload_dataset(gc.inputs(case), t.Y)
    net = _lone(gnn, case, w, max_batch)
    net.upload_dataset(*_other_rows(case))
    net.upload_held_out(gc.inputs(case), t.Y)
    assert net.held_out_size == n and net.dataset_size == 40
    hits, loss = net.evaluate_range(0, n, held_out=True)
    assert (hits, loss) == twin.evaluate_range(0, n)
    assert net.evaluate_range(held_out=True) == (hits, loss)
    assert net.evaluate_range(7, n - 9, held_out=True) == twin.evaluate_range(7, n - 9)
    conf = net.confusion_range(0, n, held_out=True)
    assert np.array_equal(conf, twin.confusion_range(0, n)) and np.trace(conf) == hits
    assert np.array_equal(net.labels_range(0, n, held_out=True), twin.labels_range(0, n))
    assert net.count_hits_range(0, n, held_out=True) == twin.count_hits_range(0, n) == hits
    assert net.evaluate_range(0, 40, held_out=False) == net.evaluate_range(0, 40)
    assert np.array_equal(net.confusion_range(0, 40, held_out=False), net.confusion_range(0, 40))
    lo, hi = t.hits_bounds(t.label[0], t.safe[0])
    assert lo <= hits <= hi
    if case.dtype == gc.F32:
        assert abs(loss - t.loss[0].sum()) <= (2e-4 * np.abs(t.loss[0]) + 2e-4).sum()
    net.close()
    twin.close()


def test_u8_encodings_of_the_held_out_set(gnn):
    rng = np.random.default_rng(3)
    pix, lab = rng.integers(0, 256, (70, 784), dtype=np.uint8), rng.integers(0, 10, 70, dtype=np.uint8)
    pix2, lab2 = rng.integers(0, 256, (33, 784), dtype=np.uint8), rng.integers(0, 10, 33, dtype=np.uint8)
    for dtype in (gnn.DTYPE_F32, gnn.DTYPE_BF16):
        net = gnn.SoftmaxCrossEntropyNeuralNet([784, 100, 50, 10], dtype=dtype, max_batch=64)
        twin = gnn.SoftmaxCrossEntropyNeuralNet([784, 100, 50, 10], dtype=dtype, max_batch=64)
        net.upload_dataset_u8(pix2, lab2)
        net.upload_held_out_u8(pix, lab)
        twin.upload_dataset_u8(pix, lab)
        assert net.evaluate_range(held_out=True) == twin.evaluate_range()
        twin.upload_dataset_u8(pix2, lab2)
        assert net.evaluate_range() == twin.evaluate_range()
        net.close()
        twin.close()
    g = gnn.NetGroup([784, 100, 50, 10], [1, 2], max_batch=64)
    tg = gnn.NetGroup([784, 100, 50, 10], [1, 2], max_batch=64)
    tr = gnn.NetGroupTrainer(pix2, lab2, g, raw_u8=True, held_out=(pix, lab))
    tg.upload_dataset_u8(pix, lab)
    assert tr.size == 33 and g.held_out_size == 70
    for a, b in zip(g.evaluate_range(held_out=True), tg.evaluate_range()):
        assert np.array_equal(a, b)
    g.close()
    tg.close()


# ---- G2: the two sets do not see each other --------------------------------------------------------------------------------------
def _case_net(gnn, case, seed=hc.SEED, max_batch=64):
    return gnn.NeuralNet(case.dims, case.kind, case.inner, case.last, gnn.LOSS_HALF_SQUARED, seed=seed, dtype=case.dtype, max_batch=max_batch)


def _train_sampled(gnn, net, sampler, iterations, batch, step, momentum):
    gnn._capi.check(net._lib.gnn_mlp_train_sampled(net._h, sampler._h, int(iterations), int(batch), float(step), float(momentum), 0))


def _same_state(a, b):
    assert np.array_equal(a.get_weights(), b.get_weights())
    assert np.array_equal(a.get_momentum(), b.get_momentum())
    assert a.time == b.time


def test_held_out_uploads_are_invisible_to_training(gnn):
    case = hc.CASES["T1"]
    X, Y = hc.training_set(case)
    Xh, Yh = hc.held_out_set(case)
    nets, samplers = [], []
    for held in (True, False):
        net, s = _case_net(gnn, case), gnn.Sampler(case.train_rows, seed=1)
        net.upload_dataset(X, Y)
        net.train_range(0, hc.BATCH, 7, case.step, hc.MOMENTUM)
        if held:
            net.upload_held_out(Xh, Yh)
            net.evaluate_range(held_out=True)
        _train_sampled(gnn, net, s, 9, hc.BATCH, case.step, hc.MOMENTUM)
        if held:
            net.upload_held_out(Xh[:31], Yh[:31])  # a replacement of another size
            assert net.held_out_size == 31
            net.confusion_range(held_out=True)
            net.labels_range(held_out=True)
        net.train_range(56, hc.BATCH, 5, case.step, hc.MOMENTUM)
        _train_sampled(gnn, net, s, 4, hc.BATCH, case.step, hc.MOMENTUM)
        nets.append(net)
        samplers.append(s)
    _same_state(*nets)
    assert nets[0].time == 25
    assert np.array_equal(samplers[0].sample(hc.BATCH), samplers[1].sample(hc.BATCH))
    # uploading the training set leaves the held-out set alone
    before = nets[0].evaluate_range(held_out=True), nets[0].labels_range(held_out=True)
    nets[0].upload_dataset(X[:50], Y[:50])
    assert nets[0].held_out_size == 31 and nets[0].dataset_size == 50
    after = nets[0].evaluate_range(held_out=True), nets[0].labels_range(held_out=True)
    assert before[0] == after[0] and np.array_equal(before[1], after[1])
    for net in nets:
        net.close()


def test_held_out_upload_keeps_a_pending_host_batch_update(gnn):
    case = hc.CASES["T1"]
    X, Y = hc.training_set(case)
    Xh, Yh = hc.held_out_set(case)
    nets = []
    for held in (True, False):
        net = _case_net(gnn, case)
        net.gradientStep(X[:8], case.step, hc.MOMENTUM, False, expected=Y[:8])     # (its update may wait for the next call)
        if held:
            net.upload_held_out(Xh, Yh)
        net.gradientStep(X[8:16], case.step, hc.MOMENTUM, False, expected=Y[8:16])
        if held:
            net.upload_held_out(Xh[:9], Yh[:9])
        nets.append(net)
    _same_state(*nets)
    for net in nets:
        net.close()


def test_group_held_out_uploads_are_invisible_to_training(gnn):
    case = hc.CASES["T1"]
    X, Y = hc.training_set(case)
    Xh, Yh = hc.held_out_set(case)
    steps, groups = [0.02, 0.015, 0.025], []
    for held in (True, False):
        g = gnn.NetGroup(case.dims, [1, 2, 3], out_kind=case.kind, inner_act=case.inner, last_act=case.last, max_batch=64)
        s = gnn.Sampler(case.train_rows, seed=1)
        g.upload_dataset(X, Y)
        g.train_range(0, hc.BATCH, 6, steps, hc.MOMENTUM)
        if held:
            g.upload_held_out(Xh, Yh)
            g.evaluate_range(held_out=True)
        g.train_sampled(s, 7, hc.BATCH, steps, hc.MOMENTUM)
        if held:
            g.upload_held_out(Xh[:20], Yh[:20])
            g.confusion_range(held_out=True)
            with pytest.raises(gnn.GnnError) as e:  # a member sees the group's set; it cannot replace it
                g.members[1].upload_held_out(Xh, Yh)
            assert e.value.code == 5
            assert g.members[1].held_out_size == 20
        g.train_range(48, hc.BATCH, 5, steps, hc.MOMENTUM)
        groups.append(g)
    for a, b in zip(groups[0].members, groups[1].members):
        _same_state(a, b)
    for g in groups:
        g.close()


# ---- G3: the held-out curve and the best weights of a lone net -------------------------------------------------------------------
def _lone_twin(gnn, case, every=hc.EVERY, iterations=hc.ITERATIONS):
    """The curve through the calls that existed before: one train_sampled call per interval, evaluate and get_weights behind it."""
    net, s = _case_net(gnn, case), gnn.Sampler(case.train_rows, seed=hc.SEED)
    net.upload_dataset(*hc.training_set(case))
    net.upload_held_out(*hc.held_out_set(case))
    hits, loss, weights, done = [], [], [], 0
    for at in hc.point_iterations(iterations, every):
        _train_sampled(gnn, net, s, at - done, hc.BATCH, case.step, hc.MOMENTUM)
        done = at
        h, l = net.evaluate_range(0, case.held_rows, held_out=True)
        hits.append(h)
        loss.append(l)
        weights.append(net.get_weights())
    return net, s, np.array(hits), np.array(loss), weights


_ORACLE_BEST = {("T1", "loss"): 4, ("T3", "loss"): 4, ("T1h", "hits"): 3, ("T2h", "hits"): 12, ("T2h", "loss"): 7, ("T3", "hits"): None}


@pytest.mark.parametrize("name", ["T1", "T1h", "T2h", "T3", "T1r", "T1b"])
@pytest.mark.parametrize("rule", ["loss", "hits"])
def test_lone_curve_and_best_weights(gnn, oracle_mod, name, rule):
    case = hc.CASES[name]
    twin, ts, t_hits, t_loss, t_w = _lone_twin(gnn, case)
    net, s = _case_net(gnn, case), gnn.Sampler(case.train_rows, seed=hc.SEED)
    tr = gnn.NeuralNetTrainer(*hc.training_set(case), net, held_out=hc.held_out_set(case))
    assert tr.size == case.train_rows and net.held_out_size == case.held_rows
    hits, loss, best, w = net.train_sampled_held_out(s, hc.ITERATIONS, hc.BATCH, case.step, hc.MOMENTUM, hc.EVERY, rule=rule)
    print(name, rule, "hits", hits.tolist(), "loss", np.round(loss, 4).tolist(), "best", best)
    assert hits.shape == loss.shape == (hc.POINTS,)
    assert np.array_equal(hits, t_hits) and np.array_equal(loss, t_loss)      # bit for bit evaluate_range at that moment
    assert best == gnn.best_point(t_hits, t_loss, rule) and best >= 0
    assert np.array_equal(w, t_w[best])                                         # bit for bit get_weights at that point
    _same_state(net, twin)                                                      # ... and the training is train_sampled's
    assert np.array_equal(s.sample(hc.BATCH), ts.sample(hc.BATCH))
    one, os_ = _case_net(gnn, case), gnn.Sampler(case.train_rows, seed=hc.SEED)  # ONE train_sampled call of 123 iterations
    one.upload_dataset(*hc.training_set(case))
    _train_sampled(gnn, one, os_, hc.ITERATIONS, hc.BATCH, case.step, hc.MOMENTUM)
    _same_state(net, one)
    if case.dtype == hc.F32 and name in ("T1", "T1h", "T2h", "T3"):
        c = hc.curve(oracle_mod, name)
        err = np.abs(loss - c.loss)
        bound = 2e-4 * np.abs(c.loss) + 2e-4 * case.held_rows
        print("  oracle loss", np.round(c.loss, 4).tolist(), "worst error / bound", float((err / bound).max()))
        assert (err <= bound).all()
        if name in ("T1h", "T2h"):
            assert np.array_equal(hits, c.hits)  # every top-2 margin is above 1e-3 (test_held_out_cpu.py)
        want = _ORACLE_BEST.get((name, rule))
        if want is not None:
            assert best == want == gnn.best_point(c.hits, c.loss, rule)
    for n_ in (net, twin, one):
        n_.close()


def test_lone_second_call_rows_rule_and_no_weights(gnn):
    """A second call on the same net continues the run: a longer history (P = 20 after 13), fewer held-out rows than uploaded, a
    point every iteration, `every` above the iterations (one point), and weights=False."""
    case = hc.CASES["T3"]
    twin, ts = _case_net(gnn, case), gnn.Sampler(case.train_rows, seed=hc.SEED)
    net, s = _case_net(gnn, case), gnn.Sampler(case.train_rows, seed=hc.SEED)
    for n_ in (net, twin):
        n_.upload_dataset(*hc.training_set(case))
        n_.upload_held_out(*hc.held_out_set(case))
    args = (hc.BATCH, case.step, hc.MOMENTUM)
    net.train_sampled_held_out(s, 33, *args, 10)
    _train_sampled(gnn, twin, ts, 33, *args)
    t_hits, t_loss, t_w = [], [], []
    for _ in range(20):
        _train_sampled(gnn, twin, ts, 1, *args)
        h, l = twin.evaluate_range(0, 37, held_out=True)
        t_hits.append(h)
        t_loss.append(l)
        t_w.append(twin.get_weights())
    hits, loss, best, w = net.train_sampled_held_out(s, 20, *args, 1, held_rows=37, rule="hits")
    assert np.array_equal(hits, t_hits) and np.array_equal(loss, t_loss)
    assert best == gnn.best_point(t_hits, t_loss, "hits") and np.array_equal(w, t_w[best])
    _same_state(net, twin)
    hits, loss, best, w = net.train_sampled_held_out(s, 5, *args, 9, weights=False)
    _train_sampled(gnn, twin, ts, 5, *args)
    assert hits.shape == (1,) and best == 0 and w is None
    assert (int(hits[0]), float(loss[0])) == twin.evaluate_range(held_out=True)
    _same_state(net, twin)
    net.close()
    twin.close()


def test_lone_nan_curve(gnn):
    """A step size that drives the net to NaN: the loss rule keeps the last point that was a number, or none."""
    case = hc.CASES["T3"]
    net, s = _case_net(gnn, case), gnn.Sampler(case.train_rows, seed=hc.SEED)
    net.upload_dataset(*hc.training_set(case))
    net.upload_held_out(*hc.held_out_set(case))
    w0 = np.full(net.n_params, np.nan)
    net.set_weights(w0)
    sentinel = np.full(net.n_params, 7.0)
    hits, loss, best, w = net.train_sampled_held_out(s, 12, hc.BATCH, case.step, hc.MOMENTUM, 5)
    assert np.isnan(loss).all() and best == -1 and w is None
    # the C call leaves best_weights unwritten when there is no best
    out_hits, out_loss, out_best = (C.c_int64 * 3)(), (C.c_double * 3)(), C.c_int32(5)
    gnn._capi.check(net._lib.gnn_mlp_train_sampled_held_out(net._h, s._h, 12, hc.BATCH, case.step, hc.MOMENTUM, 0, 5, 70, 0, out_hits, out_loss,
                                                            C.byref(out_best), sentinel.ctypes.data_as(C.POINTER(C.c_double))))
    assert out_best.value == -1 and (sentinel == 7.0).all()
    hits, loss, best, w = net.train_sampled_held_out(s, 12, hc.BATCH, case.step, hc.MOMENTUM, 5, rule="hits")
    assert best == gnn.best_point(hits, loss, "hits") == 0 and np.isnan(w).all()
    net.close()


# ---- G4: groups ----------------------------------------------------------------------------------------------------------------
_WIDE = hc.Case("T4w", [1100, 20, 10], hc.SCE, hc.LEAKY, hc.IDENTITY, 0.02, 70)  # 18 first-layer K slabs: no grouped launches
_GROUPS = [("T1", [1, 2, 3], [8, 8, 5], [0.02, 0.015, 0.025]), ("T1r", [1, 2, 3], [8, 7, 8], [0.02, 0.015, 0.025]),
           ("T3", [1, 2], [8, 8], [0.02, 0.03]), ("T1b", [1, 2], [8, 6], [0.02, 0.015]), ("T1", [1], [8], [0.02]),
           ("T4w", [1, 2], [8, 5], [0.02, 0.015])]


def _case(name):
    return _WIDE if name == "T4w" else hc.CASES[name]


def _case_group(gnn, case, seeds):
    g = gnn.NetGroup(case.dims, seeds, out_kind=case.kind, inner_act=case.inner, last_act=case.last, dtype=case.dtype, max_batch=64)
    g.upload_dataset(*hc.training_set(case))
    g.upload_held_out(*hc.held_out_set(case))
    return g, [gnn.Sampler(case.train_rows, seed=sd) for sd in seeds]


@pytest.mark.parametrize("name, seeds, batches, steps", _GROUPS, ids=["%s-K%d" % (g[0], len(g[1])) for g in _GROUPS])
@pytest.mark.parametrize("rule", ["loss", "hits"])
def test_group_curves_and_best_weights(gnn, name, seeds, batches, steps, rule):
    case, K = _case(name), len(seeds)
    twin, ts = _case_group(gnn, case, seeds)
    t_hits, t_loss, t_ens, t_w, done = [], [], [], [], 0
    for at in hc.point_iterations():
        twin.train_sampled(ts, at - done, batches, steps, hc.MOMENTUM)
        done = at
        h, l, e = twin.evaluate_range(0, case.held_rows, held_out=True)
        t_hits.append(h)
        t_loss.append(l)
        t_ens.append(e)
        t_w.append([m.get_weights() for m in twin.members])
    t_hits, t_loss = np.array(t_hits), np.array(t_loss)
    g, ss = _case_group(gnn, case, seeds)
    print(name, "K", K, "launches per step", g.launches_per_step, "evaluation launches", g.eval_launches)
    if name == "T4w":
        assert g.launches_per_step == 0
    hits, loss, ens, best, w = g.train_sampled_held_out(ss, hc.ITERATIONS, batches, steps, hc.MOMENTUM, hc.EVERY, rule=rule)
    assert hits.shape == loss.shape == (hc.POINTS, K) and ens.shape == (hc.POINTS,) and w.shape == (K, g.n_params)
    assert np.array_equal(hits, t_hits) and np.array_equal(loss, t_loss) and np.array_equal(ens, t_ens)
    for k in range(K):
        assert best[k] == gnn.best_point(t_hits[:, k], t_loss[:, k], rule) and best[k] >= 0, "member %d" % k
        assert np.array_equal(w[k], t_w[best[k]][k]), "member %d" % k
    print("  best", best.tolist())
    one, os_ = _case_group(gnn, case, seeds)  # ONE train_sampled call with a sampler and a batch size per member
    one.train_sampled(os_, hc.ITERATIONS, batches, steps, hc.MOMENTUM)
    for k in range(K):
        _same_state(g.members[k], twin.members[k])
        _same_state(g.members[k], one.members[k])
        assert np.array_equal(ss[k].sample(8), ts[k].sample(8))
    # the group goes on as a group: a second call (scalar batch size, a point every iteration) against the twin
    hits2, loss2, ens2, best2, w2 = g.train_sampled_held_out(ss, 4, 8, steps, hc.MOMENTUM, 1, held_rows=11, rule=rule, weights=False)
    for p in range(4):
        twin.train_sampled(ts, 1, [8] * K, steps, hc.MOMENTUM)
        h, l, e = twin.evaluate_range(0, 11, held_out=True)
        assert np.array_equal(hits2[p], h) and np.array_equal(loss2[p], l) and ens2[p] == e
    assert w2 is None
    for k in range(K):
        _same_state(g.members[k], twin.members[k])
    for x in (g, twin, one):
        x.close()


def test_group_cases_cover_every_route(gnn):
    """The group cases above are to cover the grouped step with the grouped evaluation (T1, T1b), interval-by-interval training
    with the grouped evaluation (T3: no grouped step launches for its shape) and with the members evaluated one after another
    (T4w)."""
    for name, want in (("T1", (2, 2)), ("T1b", (2, 2)), ("T3", (0, 2)), ("T4w", (0, 0))):
        g, _ = _case_group(gnn, _case(name), [1, 2])
        print(name, g.launches_per_step, g.eval_launches)
        assert (g.launches_per_step, g.eval_launches) == want, name
        g.close()


# ---- G5: refusals, before any step and any draw ----------------------------------------------------------------------------------
def test_refusals(gnn):
    case = hc.CASES["T1"]
    X, Y = hc.training_set(case)
    Xh, Yh = hc.held_out_set(case)
    net, s = _case_net(gnn, case), gnn.Sampler(case.train_rows, seed=1)
    lib = net._lib
    h_, l_, b_ = (C.c_int64 * 16)(), (C.c_double * 16)(), C.c_int32()

    def call(iterations=20, batch=8, step=0.02, noise=0, every=10, rows=70, rule=0, ph=h_, pl=l_, pb=C.byref(b_), sampler=s):
        return lib.gnn_mlp_train_sampled_held_out(net._h, sampler._h if sampler else None, iterations, batch, step, 0.9, noise, every, rows,
                                                  rule, ph, pl, pb, None)

    assert net.held_out_size == 0 and lib.gnn_mlp_set_rows(net._h, 0) == 0 and lib.gnn_mlp_set_rows(net._h, 2) == -1
    assert call() == 5                                            # no training set (gnn_mlp_train_sampled's refusal)
    net.upload_dataset(X, Y)
    assert lib.gnn_mlp_set_rows(net._h, 0) == case.train_rows
    assert call() == 5                                            # no held-out set
    with pytest.raises(gnn.GnnError) as e:
        net.evaluate_range(0, 4, held_out=True)
    assert e.value.code == 5
    net.upload_held_out(Xh, Yh)
    assert call(every=0) == 1 and call(every=-2) == 1
    assert call(rows=0) == 1 and call(rows=71) == 1 and call(rows=-1) == 1
    assert call(ph=None) == 1 and call(pl=None) == 1 and call(pb=None) == 1
    assert call(rule=2) == 1 and call(rule=-1) == 1
    assert call(noise=1) == 3
    assert call(iterations=0) == 1 and call(batch=0) == 1 and call(batch=case.train_rows) == 1 and call(step=0.0) == 1 and call(sampler=None) == 1
    other = gnn.Sampler(case.train_rows + 1, seed=1)
    assert call(sampler=other) == 1                               # sampler size differs from the training set
    assert lib.gnn_mlp_evaluate_set_range(net._h, 2, 0, 4, h_, l_, None, None) == 1
    assert lib.gnn_mlp_evaluate_set_range(net._h, 1, 0, 4, None, None, None, None) == 1
    for first, cnt in ((0, 0), (-1, 4), (67, 4), (70, 1), (0, 71)):
        assert lib.gnn_mlp_evaluate_set_range(net._h, 1, first, cnt, h_, l_, None, None) == 1
    assert lib.gnn_mlp_evaluate_set_range(net._h, 0, 0, 71, h_, l_, None, None) == 0   # ... rows of the training set
    # nothing stepped, nothing drawn
    fresh = gnn.Sampler(case.train_rows, seed=1)
    assert net.time == 0 and np.array_equal(s.sample(8), fresh.sample(8))
    net.close()

    g, ss = _case_group(gnn, case, [1, 2])
    gl = g._lib
    arr = (C.c_void_p * 2)(*[x._h for x in ss])
    bs, st, mo = (C.c_int32 * 2)(8, 8), (C.c_double * 2)(0.02, 0.02), (C.c_double * 2)(0.9, 0.9)
    hh, ll, ee, bb = (C.c_int64 * 64)(), (C.c_double * 64)(), (C.c_int64 * 32)(), (C.c_int32 * 2)()

    def gcall(samplers=arr, batches=bs, noise=0, every=10, rows=70, rule=0, ph=hh, pl=ll, pb=bb):
        return gl.gnn_mlp_group_train_sampled_held_out(g._h, samplers, 20, batches, st, mo, noise, every, rows, rule, ph, pl, ee, pb, None)

    assert gcall(every=0) == 1 and gcall(rows=0) == 1 and gcall(rows=71) == 1 and gcall(rule=2) == 1
    assert gcall(ph=None) == 1 and gcall(pl=None) == 1 and gcall(pb=None) == 1
    assert gcall(noise=1) == 3
    assert gcall(samplers=None) == 1 and gcall(batches=None) == 1
    assert gcall(samplers=(C.c_void_p * 2)(ss[0]._h, ss[0]._h)) == 1          # the same sampler for two members
    assert gcall(batches=(C.c_int32 * 2)(8, 0)) == 1
    for set_ in (2, -1):
        assert gl.gnn_mlp_group_evaluate_set_range(g._h, set_, 0, 4, hh, ll, ee) == 1
        assert gl.gnn_mlp_group_ensemble_set_range(g._h, set_, 0, 4, ll, None) == 1
        assert gl.gnn_mlp_group_confusion_set_range(g._h, set_, 0, 4, hh, None, None) == 1
    with pytest.raises(gnn.GnnError) as e:
        g.evaluate_range(60, 11, held_out=True)
    assert e.value.code == 1
    assert all(m.time == 0 for m in g.members)
    assert np.array_equal(ss[0].sample(8), gnn.Sampler(case.train_rows, seed=1).sample(8))
    g.close()
    g2 = gnn.NetGroup(case.dims, [1, 2], inner_act=case.inner, max_batch=64)
    g2.upload_dataset(X, Y)
    with pytest.raises(gnn.GnnError) as e:   # no held-out set
        g2.evaluate_range(0, 4, held_out=True)
    assert e.value.code == 5
    with pytest.raises(gnn.GnnError) as e:
        g2.train_sampled_held_out([gnn.Sampler(case.train_rows, 1), gnn.Sampler(case.train_rows, 2)], 20, 8, 0.02, 0.9, 10, held_rows=5)
    assert e.value.code == 5
    g2.close()


def test_log_run_writes_both_accuracies(gnn, tmp_path):
    case = hc.CASES["T3"]
    net = _case_net(gnn, case)
    tr = gnn.NeuralNetTrainer(*hc.training_set(case), net, held_out=hc.held_out_set(case))
    tr.train(30, case.step, hc.BATCH, hc.MOMENTUM)
    path = tmp_path / "logs" / "trainLog.csv"
    train_acc, test_acc = tr.log_run(path, case.dims, 30, case.step, hc.BATCH, hc.MOMENTUM)
    assert train_acc == net.count_hits_range() / case.train_rows and test_acc == net.evaluate_range(held_out=True)[0] / 70
    assert path.read_text() == gnn.train_log_row(case.dims, 30, case.step, hc.BATCH, hc.MOMENTUM, False, train_acc, test_acc)
    assert path.read_text().startswith("24-136-10,30,0.02000,8,0.900,false,")
    net.close()
