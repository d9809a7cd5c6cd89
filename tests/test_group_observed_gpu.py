"""NetGroup.train_sampled_observed / gnn_mlp_group_train_sampled_observed: the observed loop NNT:68-79 of every member of a group,
its validation pass as ONE grouped launch per iteration (the LOSS_ONLY form of group_forward_kernel) and the curves summed on the
device (group_curve_sum_kernel) -- or member after member where a group has no grouped launches.

Every equality is against a form the library already has: a twin group that makes the same calls with train_sampled (weights,
momentum, time bit for bit; the samplers' next draws), a twin stepped one iteration per call with evaluate_range behind each
(the curve, to (alpha) of tests/group_observed_cases.py), the lone handle's gnn_mlp_train_sampled_observed (bit for bit, on the
member-after-member route), and the fp64 oracle at the one configuration whose budget (beta) the project has."""
import ctypes as C
import io

import numpy as np
import pytest

from tests import chain_cases as cc
from tests import group_observed_cases as oc

pytestmark = pytest.mark.gpu

A = [784, 300, 100, 10]
Bn = [784, 100, 50, 10]


class _Setup:
    """How to make identical groups of one configuration: the nets, their start weights, the data set."""

    def __init__(self, gnn, dims, K, X, Y, max_batch, dtype=0, out_kind=0, inner=None, last=None, w_scale=1.0):
        self.gnn, self.dims, self.K, self.X, self.Y, self.max_batch, self.dtype = gnn, dims, K, X, Y, max_batch, dtype
        self.out_kind = out_kind
        self.inner = gnn.ACT_LEAKY_RELU if inner is None else inner
        self.last = gnn.ACT_IDENTITY if last is None or out_kind == cc.OUT_SOFTMAX_CE else last
        self.w_scale, self.w0 = w_scale, None
        self.N = X.shape[0]

    def group(self, max_batch=None):
        g = self.gnn.NetGroup(self.dims, list(range(1, self.K + 1)), out_kind=self.out_kind, inner_act=self.inner, last_act=self.last,
                              dtype=self.dtype, max_batch=max_batch or self.max_batch)
        if self.w0 is None:
            self.w0 = [m.get_weights() * self.w_scale for m in g.members]
        for m, w in zip(g.members, self.w0):
            m.set_weights(w)
        g.upload_dataset(self.X, self.Y)
        return g

    def lone(self, k):
        gnn = self.gnn
        if self.out_kind == cc.OUT_SOFTMAX_CE:
            n = gnn.SoftmaxCrossEntropyNeuralNet(self.dims, inner_act=self.inner, seed=k + 1, dtype=self.dtype, max_batch=self.max_batch)
        else:
            n = gnn.GeneralNeuralNet(self.dims, inner_act=self.inner, last_act=self.last, seed=k + 1, dtype=self.dtype, max_batch=self.max_batch)
        n.set_weights(self.w0[k])
        n.upload_dataset(self.X, self.Y)
        return n


def _drawn(gnn, seed, dtype, K):
    dims, B, inner, out_kind, last = cc.chain_case(seed)
    X, Y = cc.chain_data(seed, dims, B)
    return _Setup(gnn, dims, K, X, Y, B, dtype, out_kind, inner, last, cc.W_SCALE), B


def _same_members(g, t, what=""):
    for k, (a, b) in enumerate(zip(g.members, t.members)):
        assert np.array_equal(a.get_weights(), b.get_weights()), "weights differ, member %d %s" % (k, what)
        assert np.array_equal(a.get_momentum(), b.get_momentum()), "momentum differs, member %d %s" % (k, what)
        assert a.time == b.time, "time differs, member %d %s" % (k, what)


def _run(g, s, segments, B, steps, moms, lone_step, call):
    """The tests' call sequence on group g: call(n) per segment; between two segments member 0 alone takes a step on a host
    batch, so that the group finds its members' look-ahead states unequal."""
    out = []
    for i, n in enumerate(segments):
        if i and lone_step is not None:
            g.members[0].gradientStep(lone_step[0], oc.LONE_STEP[0], oc.LONE_STEP[1], False, expected=lone_step[1])
        out.append(call(n))
    return out


def _grouped_rules(setup, B, V, segments, steps, moms, lone_step, what):
    """The rules of the grouped route; returns the observed group and its curve (the caller closes the group)."""
    gnn, N, K = setup.gnn, setup.N, setup.K
    g, t, p = setup.group(), setup.group(), setup.group()
    sg, st, sp = (gnn.Sampler(N, seed=cc.SAMPLER_SEED) for _ in range(3))
    assert g.launches_per_step == 2 and g.observed_launches == 3
    curve = np.concatenate(_run(g, sg, segments, B, steps, moms, lone_step,
                                lambda n: g.train_sampled_observed(sg, n, B, steps, moms, V)))
    assert curve.shape == (sum(segments), K)
    # the same calls without observation: the members and the sampler end in the same state
    _run(t, st, segments, B, steps, moms, lone_step, lambda n: t.train_sampled(st, n, B, steps, moms))
    _same_members(g, t, what)
    assert np.array_equal(sg.sample(B), st.sample(B))

    # one iteration per call, evaluate_range behind each
    def stepwise(n):
        rows = []
        for _ in range(n):
            p.train_sampled(sp, 1, B, steps, moms)
            rows.append(p.evaluate_range(0, V)[1] / V)
        return np.array(rows)
    ref = np.concatenate(_run(p, sp, segments, B, steps, moms, lone_step, stepwise))
    _same_members(p, t, what + " (stepwise twin)")
    err = np.abs(curve - ref) / np.abs(ref)
    print(what, "V", V, "curve range", curve.min(), curve.max(), "largest relative distance to the per-iteration form", err.max())
    assert oc.close_alpha(curve, ref), (what, err.max())
    assert oc.close_alpha(g.evaluate_range(0, V)[1] / V, curve[-1]), what
    for x in (t, p, sg, st, sp):
        x.close()
    return g, curve


def _lone_observed(lone, s, n, B, step, mom, V):
    val = np.empty(n)
    rc = lone._lib.gnn_mlp_train_sampled_observed(lone._h, s._h, n, B, step, mom, 0, V, val.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == 0
    return val


def _member_rules(setup, B, V, segments, steps, moms, lone_step, what):
    """The rules of the member-after-member route."""
    gnn, N, K = setup.gnn, setup.N, setup.K
    g, t = setup.group(), setup.group()
    sg, st = gnn.Sampler(N, seed=cc.SAMPLER_SEED), gnn.Sampler(N, seed=cc.SAMPLER_SEED)
    assert g.observed_launches == 0
    curve = np.concatenate(_run(g, sg, segments, B, steps, moms, lone_step,
                                lambda n: g.train_sampled_observed(sg, n, B, steps, moms, V)))
    _run(t, st, segments, B, steps, moms, lone_step, lambda n: t.train_sampled(st, n, B, steps, moms))
    _same_members(g, t, what)
    assert np.array_equal(sg.sample(B), st.sample(B))
    assert np.isfinite(curve).all()
    for k in range(K):
        lone, ls = setup.lone(k), gnn.Sampler(N, seed=cc.SAMPLER_SEED)
        col = []
        for i, n in enumerate(segments):
            if i and k == 0 and lone_step is not None:
                lone.gradientStep(lone_step[0], oc.LONE_STEP[0], oc.LONE_STEP[1], False, expected=lone_step[1])
            col.append(_lone_observed(lone, ls, n, B, steps[k], moms[k], V))
        assert np.array_equal(curve[:, k], np.concatenate(col)), "%s: column %d is not the lone handle's curve" % (what, k)
        assert np.array_equal(g.members[k].get_weights(), lone.get_weights()), "%s: member %d" % (what, k)
        lone.close(); ls.close()
    for x in (g, t, sg, st):
        x.close()


def _drawn_case(gnn, seed, dtype, K, route=None):
    setup, B = _drawn(gnn, seed, dtype, K)
    V = oc.validation_rows(B)
    steps, moms = oc.case_hyper(K)
    lone_step = (setup.X[B:2 * B], setup.Y[B:2 * B])
    what = oc.id_of((seed, dtype, K))
    if route is None:
        probe = setup.group()
        route = 0 if probe.launches_per_step == 0 or K == 1 else 2
        print(what, "launches_per_step", probe.launches_per_step, "observed_launches", probe.observed_launches)
        probe.close()
    if route == 2:
        g, _ = _grouped_rules(setup, B, V, oc.SEGMENTS, steps, moms, lone_step, what)
        g.close()
    else:
        _member_rules(setup, B, V, oc.SEGMENTS, steps, moms, lone_step, what)


@pytest.mark.parametrize("seed,dtype,K", oc.GROUPED_CASES, ids=[oc.id_of(c) for c in oc.GROUPED_CASES])
def test_drawn_cases_grouped_route(gnn, seed, dtype, K):
    """observed(17); a lone host-batch step on member 0; observed(7) at V = N - 3 on the drawn shapes: three launches per
    iteration, the members and the sampler as after train_sampled, the curve that of the per-iteration form."""
    _drawn_case(gnn, seed, dtype, K, route=2)


@pytest.mark.parametrize("seed,dtype,K", oc.MEMBER_ROUTE_CASES, ids=[oc.id_of(c) for c in oc.MEMBER_ROUTE_CASES])
def test_member_after_member_route(gnn, seed, dtype, K):
    """Groups without grouped step launches and a group of one net: column k is bit for bit the lone handle's curve.  (The bf16
    group's route is read from launches_per_step; where that is 2 the rules of the grouped route apply.)"""
    fixed = (seed, dtype, K) in oc.FALLBACK_CASES or K == 1
    _drawn_case(gnn, seed, dtype, K, route=0 if fixed else None)


class _Monitor:
    def __init__(self):
        self.steps = self.finished = 0

    def step(self):
        self.steps += 1

    def finish(self):
        self.finished += 1


def test_against_the_fp64_oracle_through_the_trainer(gnn, oracle_mod):
    """784-100-50-10 f32, three members with their own seeds, steps and momenta, 12 iterations: every val[i][k] within (beta) of
    the oracle's validate() on the oracle's own trajectory of member k, at V = 7 (NetGroupTrainer's own, N // 100 + 1) and
    V = 150; the observers' text is "%d,%.2f" of the same values; a monitor is stepped once per iteration."""
    pix, lab, _, _ = oc.oracle_data()
    truth = oc.oracle_curves(oracle_mod)
    K, it, B = len(oc.ORACLE_SEEDS), oc.ORACLE_ITERATIONS, oc.ORACLE_B
    raw = {}
    for V in oc.ORACLE_V:
        g = gnn.NetGroup(oc.ORACLE_DIMS, oc.ORACLE_SEEDS, max_batch=B)
        tr = gnn.NetGroupTrainer(pix, lab, g, raw_u8=True)
        assert tr.size == oc.ORACLE_N and g.observed_launches == 3
        raw[V] = g.train_sampled_observed(tr.sampler, it, B, oc.ORACLE_STEPS, oc.ORACLE_MOMENTA, validation_size=V)
        units = np.abs(raw[V] - truth[V]) / oc.budget(truth[V])
        print("V", V, "largest distance to the oracle in budgets, per member:", units.max(axis=0))
        assert np.isfinite(raw[V]).all() and (units <= 1).all(), (V, units.max())
        g.close()
    g = gnn.NetGroup(oc.ORACLE_DIMS, oc.ORACLE_SEEDS, max_batch=B)
    tr = gnn.NetGroupTrainer(pix, lab, g, raw_u8=True)
    tr.OBSERVER_BURST = 5                                         # three device loops: 5 + 5 + 2 iterations
    streams, mon = [io.StringIO() for _ in range(K)], _Monitor()
    tr.train(it, oc.ORACLE_STEPS, B, oc.ORACLE_MOMENTA, False, monitor=mon, observers=streams)
    assert mon.steps == it and mon.finished == 1
    assert [m.time for m in g.members] == [it] * K
    for k in range(K):
        assert streams[k].getvalue() == "".join("%d,%.2f\n" % (i, raw[7][i, k]) for i in range(it))
    # no observers: train_sampled, the same weights
    g2 = gnn.NetGroup(oc.ORACLE_DIMS, oc.ORACLE_SEEDS, max_batch=B)
    tr2 = gnn.NetGroupTrainer(pix, lab, g2, raw_u8=True)
    m2 = _Monitor()
    tr2.train(it, oc.ORACLE_STEPS, B, oc.ORACLE_MOMENTA, False, monitor=m2)
    assert m2.steps == it and m2.finished == 1
    _same_members(g, g2)
    with pytest.raises(ValueError):
        tr2.train(3, 0.01, B, 0.9, observers=streams[:2])
    g.close(); g2.close()


def test_curve_matrix_is_summed_and_refilled(gnn):
    """300 iterations in ONE call: the 256-row curve matrix is summed, refilled, and summed again behind the last step; sampler
    chunks of 16, 32, 64 and 128 iterations (and a last one of 60)."""
    seed, dtype, K = oc.REFILL_CASE
    setup, B = _drawn(gnn, seed, dtype, K)
    steps, moms = oc.case_hyper(K)
    g, curve = _grouped_rules(setup, B, oc.REFILL_V, (oc.REFILL_ITERATIONS,), steps, moms, None, "refill " + oc.id_of(oc.REFILL_CASE))
    assert curve.shape == (oc.REFILL_ITERATIONS, K)
    g.close()


@pytest.mark.parametrize("dims,dtype,K", [(A, 0, 3), (A, 1, 16), (Bn, 0, 8)], ids=["784-300-100-10-f32-K3", "784-300-100-10-bf16-K16", "784-100-50-10-f32-K8"])
def test_prebuilt_instances(gnn, dims, dtype, K, monkeypatch):
    """The prebuilt shapes at the trainer's own validation size for MNIST (V = 601): 25 iterations of batch 96 over 1000 rows
    (refills shorten batches).  And, for the first configuration, validation in 19 blocks of 32 rows against validation in
    one block: the same curve to (alpha), the same weights -- with batches of 32 for both groups, the most a group created
    with max_batch = 32 steps."""
    N, batch, V = 1000, 96, 601
    rng = np.random.default_rng(3)
    X, Y = rng.random((N, 784)), np.eye(10)[rng.integers(0, 10, N)]
    setup = _Setup(gnn, dims, K, X, Y, batch, dtype, w_scale=0.5)
    steps, moms = [0.01 + 0.004 * k / K for k in range(K)], [0.9 - 0.05 * k / K for k in range(K)]
    g, curve = _grouped_rules(setup, batch, V, (18, 7), steps, moms, (X[batch:2 * batch], Y[batch:2 * batch]),
                              "prebuilt %s dtype %d K %d" % ("-".join(map(str, dims)), dtype, K))
    assert g.members[0].rowblock_state == 2  # the prebuilt static instance
    g.close()
    if (dims, dtype) == (A, 0):
        one = setup.group()
        monkeypatch.setenv("GNN_MLP_EVAL_ROWS", "0")
        many = setup.group(max_batch=32)
        monkeypatch.delenv("GNN_MLP_EVAL_ROWS")
        assert many.observed_launches == 3
        s1, s2 = gnn.Sampler(N, seed=1), gnn.Sampler(N, seed=1)
        c1 = one.train_sampled_observed(s1, 25, 32, steps, moms, V)
        c2 = many.train_sampled_observed(s2, 25, 32, steps, moms, V)
        print("19 blocks against one: largest relative distance", (np.abs(c2 - c1) / np.abs(c1)).max())
        assert oc.close_alpha(c2, c1)
        _same_members(many, one, "(19 validation blocks)")
        for x in (one, many, s1, s2):
            x.close()


def test_refusals(gnn):
    lib = gnn.load_library()
    N, B, K, V = 300, 32, 2, 4
    rng = np.random.default_rng(5)
    X, Y = rng.random((N, 784)), np.eye(10)[rng.integers(0, 10, N)]
    setup = _Setup(gnn, Bn, K, X, Y, 64)
    g, t = setup.group(), setup.group()
    sg, st, other = gnn.Sampler(N, seed=1), gnn.Sampler(N, seed=1), gnn.Sampler(N + 1, seed=1)
    dp = C.POINTER(C.c_double)
    arr = (C.c_double * K)(0.01, 0.02)
    mom = (C.c_double * K)(0.9, 0.8)
    val = np.empty((3, K))
    out = val.ctypes.data_as(dp)
    call = lib.gnn_mlp_group_train_sampled_observed
    refusals = [
        ("null val_loss", lambda: call(g._h, sg._h, 3, B, arr, mom, 0, V, None), 1),
        ("null steps", lambda: call(g._h, sg._h, 3, B, None, mom, 0, V, out), 1),
        ("null momenta", lambda: call(g._h, sg._h, 3, B, arr, None, 0, V, out), 1),
        ("validation_size 0", lambda: call(g._h, sg._h, 3, B, arr, mom, 0, 0, out), 1),
        ("validation_size N + 1", lambda: call(g._h, sg._h, 3, B, arr, mom, 0, N + 1, out), 1),
        ("noise", lambda: call(g._h, sg._h, 3, B, arr, mom, 1, V, out), 3),
        ("a sampler of another size", lambda: call(g._h, other._h, 3, B, arr, mom, 0, V, out), 1),
    ]
    assert call(None, sg._h, 3, B, arr, mom, 0, V, out) == 1 and lib.gnn_mlp_group_observed_launches(None) == -1
    for what, refused, code in refusals:
        assert refused() == code, what
        # nothing was stepped, nothing drawn: the group still trains and stays its twin
        c = g.train_sampled_observed(sg, 3, B, [0.01, 0.02], [0.9, 0.8], V)
        t.train_sampled(st, 3, B, [0.01, 0.02], [0.9, 0.8])
        assert np.isfinite(c).all() and c.shape == (3, K)
        _same_members(g, t, "(after: %s)" % what)
    assert np.array_equal(sg.sample(B), st.sample(B))
    with pytest.raises(ValueError):
        g.train_sampled_observed(sg, 3, B, [0.01], 0.9, V)
    for x in (g, t, sg, st, other):
        x.close()
