"""A NetGroup trained with ONE SAMPLER PER MEMBER (gnn_mlp_group_train_sampled_each; NetGroup.train_sampled([s_0 .. s_{K-1}], ..)).

The one rule: member k is, bit for bit (weights, momentum, time), the lone net created with seeds[k] after gnn_mlp_train_sampled
with a fresh sampler of s_k's seed; every s_k's next draw is the lone run's sampler's next draw; and
NetGroup.sampled_each_iterations is what tests/test_group_samplers_cpu.py predicts from the CPU oracle's sampler -- the
fixtures there have iterations whose batch sizes differ between the members (stepped member after member) between iterations
stepped by the grouped launches."""
import ctypes as C
import io

import numpy as np
import pytest

from tests import group_observed_cases as oc
from tests import test_group_samplers_cpu as fx

pytestmark = pytest.mark.gpu

Bn = [784, 100, 50, 10]       # prebuilt instances
SMALL = [65, 20, 12, 5]       # runtime-shape instances, one ragged 4-row block (the net of tests/test_launch_counts_gpu.py)
OFF_PATH = [784, 1024, 1024, 1024, 10]


def _data(n, d_in, d_out, seed=0):
    rng = np.random.default_rng(seed)
    return rng.random((n, d_in)), np.eye(d_out)[rng.integers(0, d_out, n)]


def _hyper(k):
    return [0.01 + 0.004 * i for i in range(k)], [0.9 - 0.05 * i for i in range(k)]


def _lone(gnn, monkeypatch, kind, dims, seed, dtype, max_batch):
    with monkeypatch.context() as m:
        m.setenv("GNN_MLP_JIT", "0")
        if kind == "sce":
            return gnn.SoftmaxCrossEntropyNeuralNet(dims, seed=seed, dtype=dtype, max_batch=max_batch)
        return gnn.GeneralNeuralNet(dims, inner_act="sigmoid", last_act="sigmoid", seed=seed, dtype=dtype, max_batch=max_batch)


def _group(gnn, monkeypatch, kind, dims, seeds, dtype, max_batch):
    with monkeypatch.context() as m:
        m.setenv("GNN_MLP_JIT", "0")
        if kind == "sce":
            return gnn.NetGroup(dims, seeds, dtype=dtype, max_batch=max_batch)
        return gnn.NetGroup(dims, seeds, out_kind=gnn.OUT_ACT_LOSS, inner_act="sigmoid", last_act="sigmoid", dtype=dtype,
                            max_batch=max_batch)


def _samplers(gnn, name, seeds=None):
    N, batch, _, sseeds, advance = fx.FIXTURES[name]
    out = []
    for k, seed in enumerate(sseeds if seeds is None else seeds):
        s = gnn.Sampler(N, seed=seed)
        if advance and advance[k]:
            s.sample(advance[k])
        out.append(s)
    return out


def _assert_same(member, lone, what=""):
    assert np.array_equal(member.get_weights(), lone.get_weights()), "weights differ " + what
    assert np.array_equal(member.get_momentum(), lone.get_momentum()), "momentum differs " + what
    assert member.time == lone.time, "time differs " + what


def _lone_sampled(lone, s, n, batch, step, mom):
    assert lone._lib.gnn_mlp_train_sampled(lone._h, s._h, n, batch, step, mom, 0) == 0


def _lone_observed(lone, s, n, batch, step, mom, V):
    val = np.empty(n)
    rc = lone._lib.gnn_mlp_train_sampled_observed(lone._h, s._h, n, batch, step, mom, 0, V, val.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == 0
    return val


def _one_rule(gnn, monkeypatch, oracle_mod, name, kind, dims, dtype, wseeds, calls=None, expect_grouped=True):
    """The fixture's calls on a group and on the lone nets; returns what sampled_each_iterations said after each call."""
    N, batch, iters, sseeds, _ = fx.FIXTURES[name]
    calls = [iters] if calls is None else calls
    K = len(wseeds)
    assert K == len(sseeds)
    X, Y = _data(N, dims[0], dims[-1])
    steps, moms = _hyper(K)
    g = _group(gnn, monkeypatch, kind, dims, wseeds, dtype, batch)
    assert g.launches_per_step == (2 if expect_grouped else 0)
    g.upload_dataset(X, Y)
    ss = _samplers(gnn, name)
    said, skip = [], 0
    for n in calls:
        g.train_sampled(ss, n, batch, steps, moms)
        said.append(g.sampled_each_iterations)
        want, _ = fx.predict(oracle_mod, name, n, skip)
        assert said[-1] == (want if expect_grouped else (0, n)), (name, n, skip)
        skip += n
    ls = _samplers(gnn, name)
    for k in range(K):
        lone = _lone(gnn, monkeypatch, kind, dims, wseeds[k], dtype, batch)
        lone.upload_dataset(X, Y)
        for n in calls:
            _lone_sampled(lone, ls[k], n, batch, steps[k], moms[k])
        _assert_same(g.members[k], lone, "(%s member %d)" % (name, k))
        assert np.array_equal(ss[k].sample(batch), ls[k].sample(batch)), "sampler %d ends elsewhere" % k
        lone.close()
    for x in ss + ls + [g]:
        x.close()
    return said


# 1
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
def test_prebuilt_shape_two_calls(gnn, monkeypatch, oracle_mod, dtype):
    said = _one_rule(gnn, monkeypatch, oracle_mod, "F1", "sce", Bn, dtype, [1, 2, 3], calls=[13, 6])
    assert said[0][0] > 0 and said[0][1] > 0  # grouped and mixed iterations in the first call


# 2
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
def test_runtime_shape_ragged_block(gnn, monkeypatch, oracle_mod, dtype):
    _one_rule(gnn, monkeypatch, oracle_mod, "F2", "sce", SMALL, dtype, [1, 2, 3])


# 3
def test_general_net_group(gnn, monkeypatch, oracle_mod):
    _one_rule(gnn, monkeypatch, oracle_mod, "F2", "gnn", SMALL, 0, [1, 2, 3])


# 4
def test_sixteen_members(gnn, monkeypatch, oracle_mod):
    """K = 16: slice 15 of the index region and the last grid row are live (member 15 and sampler 15 obey the one rule)."""
    _one_rule(gnn, monkeypatch, oracle_mod, "F3", "sce", SMALL, 0, list(range(1, 17)))


# 5
def test_samplers_advanced_before_the_call(gnn, monkeypatch, oracle_mod):
    _one_rule(gnn, monkeypatch, oracle_mod, "F4", "sce", SMALL, 0, [1, 2, 3])


# 5b
@pytest.mark.parametrize("calls", [[260], [17, 243]], ids=["one-call", "cut-at-17"])
def test_across_chunk_boundaries_and_the_rings_wrap(gnn, monkeypatch, oracle_mod, calls):
    """F5: 260 iterations are five sampler chunks of the loop (they begin at 0, 16, 48, 112, 240), the fifth in ring slot 0 again;
    every chunk holds iterations stepped member after member, iteration 16 -- the first of chunk 1 -- among them
    (tests/test_group_samplers_cpu.py).  Cut at 17, the second call's chunks lie elsewhere in the samplers' sequences."""
    assert sum(calls) == fx.FIXTURES["F5"][2]
    said = _one_rule(gnn, monkeypatch, oracle_mod, "F5", "sce", SMALL, 0, [1, 2, 3], calls=calls)
    assert all(grouped > 0 and mixed > 0 for grouped, mixed in said)


# 6
def test_mixed_with_the_other_group_calls(gnn, monkeypatch, oracle_mod):
    N, batch, _, sseeds, _ = fx.FIXTURES["F2"]
    K = len(sseeds)
    X, Y = _data(N, SMALL[0], SMALL[-1])
    steps, moms = _hyper(K)
    g = _group(gnn, monkeypatch, "sce", SMALL, [1, 2, 3], 0, batch)
    g.upload_dataset(X, Y)
    shared, ss = gnn.Sampler(N, seed=5), _samplers(gnn, "F2")
    g.train_sampled(shared, 5, batch, steps, moms)
    g.train_sampled(ss, 9, batch, steps, moms)
    assert g.sampled_each_iterations == fx.predict(oracle_mod, "F2", 9)[0]
    g.members[1].gradient_step_range(3, batch, 0.02, 0.8)  # one member alone between two own-sampler calls
    g.train_sampled(ss, 4, batch, steps, moms)
    assert g.sampled_each_iterations == fx.predict(oracle_mod, "F2", 4, skip=9)[0]
    g.train_range(0, batch, 3, steps, moms)
    g.train_sampled(ss, 6, batch, steps, moms)
    assert g.sampled_each_iterations == fx.predict(oracle_mod, "F2", 6, skip=13)[0]
    ls = _samplers(gnn, "F2")
    for k in range(K):
        lone = _lone(gnn, monkeypatch, "sce", SMALL, k + 1, 0, batch)
        lone.upload_dataset(X, Y)
        lshared = gnn.Sampler(N, seed=5)
        _lone_sampled(lone, lshared, 5, batch, steps[k], moms[k])
        _lone_sampled(lone, ls[k], 9, batch, steps[k], moms[k])
        if k == 1:
            lone.gradient_step_range(3, batch, 0.02, 0.8)
        _lone_sampled(lone, ls[k], 4, batch, steps[k], moms[k])
        lone.train_range(0, batch, 3, steps[k], moms[k])
        _lone_sampled(lone, ls[k], 6, batch, steps[k], moms[k])
        _assert_same(g.members[k], lone, "(member %d)" % k)
        assert np.array_equal(ss[k].sample(batch), ls[k].sample(batch))
        for x in (lone, lshared):
            x.close()
    for x in ss + ls + [shared, g]:
        x.close()


# 7
@pytest.mark.parametrize("V", sorted({3, 203 // 100 + 1}))
def test_observed(gnn, monkeypatch, oracle_mod, V):
    N, batch, iters, sseeds, _ = fx.FIXTURES["F1"]
    K = len(sseeds)
    X, Y = _data(N, Bn[0], Bn[-1])
    steps, moms = _hyper(K)
    g, t, p = (_group(gnn, monkeypatch, "sce", Bn, [1, 2, 3], 0, batch) for _ in range(3))
    for x in (g, t, p):
        x.upload_dataset(X, Y)
    assert g.launches_per_step == 2 and g.observed_launches == 3
    sg, st, sp = (_samplers(gnn, "F1") for _ in range(3))
    curve = g.train_sampled_observed(sg, iters, batch, steps, moms, V)
    assert curve.shape == (iters, K)
    assert g.sampled_each_iterations == fx.predict(oracle_mod, "F1")[0]
    t.train_sampled(st, iters, batch, steps, moms)  # unobserved: members and samplers end in the same state
    for k in range(K):
        _assert_same(g.members[k], t.members[k], "(member %d)" % k)
        assert np.array_equal(sg[k].sample(batch), st[k].sample(batch))
    ref = []
    for _ in range(iters):  # a twin stepped one iteration per call, evaluate_range behind each
        p.train_sampled(sp, 1, batch, steps, moms)
        ref.append(p.evaluate_range(0, V)[1] / V)
    ref = np.array(ref)
    for k in range(K):
        _assert_same(p.members[k], t.members[k], "(stepwise twin, member %d)" % k)
    print("V", V, "largest relative distance to the per-iteration form", (np.abs(curve - ref) / np.abs(ref)).max())
    assert oc.close_alpha(curve, ref)
    for x in sg + st + sp + [g, t, p]:
        x.close()


# 8
@pytest.mark.parametrize("dims,K,N,batch,iters", [(SMALL, 1, 40, 12, 14), (OFF_PATH, 2, 100, 32, 4)], ids=["one-member", "off-the-two-launch-path"])
def test_fallbacks(gnn, monkeypatch, dims, K, N, batch, iters):
    X, Y = _data(N, dims[0], dims[-1])
    steps, moms = _hyper(K)
    V = 3
    g, o = (_group(gnn, monkeypatch, "sce", dims, list(range(1, K + 1)), 0, batch) for _ in range(2))
    assert g.launches_per_step == (2 if K == 1 else 0)  # (a group of one takes the member route whatever its net)
    for x in (g, o):
        x.upload_dataset(X, Y)
    ss, so, ls, lo = ([gnn.Sampler(N, seed=k + 1) for k in range(K)] for _ in range(4))
    g.train_sampled(ss, iters, batch, steps, moms)
    assert g.sampled_each_iterations == (0, iters)
    curve = o.train_sampled_observed(so, iters, batch, steps, moms, V)
    assert o.sampled_each_iterations == (0, iters) and curve.shape == (iters, K)
    for k in range(K):
        lone, lobs = (_lone(gnn, monkeypatch, "sce", dims, k + 1, 0, batch) for _ in range(2))
        for x in (lone, lobs):
            x.upload_dataset(X, Y)
        _lone_sampled(lone, ls[k], iters, batch, steps[k], moms[k])
        col = _lone_observed(lobs, lo[k], iters, batch, steps[k], moms[k], V)
        _assert_same(g.members[k], lone, "(member %d)" % k)
        _assert_same(o.members[k], lobs, "(observed, member %d)" % k)
        assert np.array_equal(curve[:, k], col)  # bit for bit the lone curve
        assert np.array_equal(ss[k].sample(batch), ls[k].sample(batch)) and np.array_equal(so[k].sample(batch), lo[k].sample(batch))
        for x in (lone, lobs):
            x.close()
    for x in ss + so + ls + lo + [g, o]:
        x.close()


# 9
def test_refusals(gnn, monkeypatch):
    lib = gnn.load_library()
    N, batch, K, V = 40, 12, 3, 3
    X, Y = _data(N, SMALL[0], SMALL[-1])
    g, t = (_group(gnn, monkeypatch, "sce", SMALL, [1, 2, 3], 0, batch) for _ in range(2))
    for x in (g, t):
        x.upload_dataset(X, Y)
    ss, st = ([gnn.Sampler(N, seed=k + 1) for k in range(K)] for _ in range(2))
    other = gnn.Sampler(N + 1, seed=1)
    arr, mom = (C.c_double * K)(0.01, 0.02, 0.03), (C.c_double * K)(0.9, 0.8, 0.7)
    val = np.empty((3, K))
    out = val.ctypes.data_as(C.POINTER(C.c_double))
    H = lambda *s: (C.c_void_p * K)(*[x._h if x is not None else None for x in s])
    call = lib.gnn_mlp_group_train_sampled_each
    refusals = [
        ("null samplers", lambda: call(g._h, None, 3, batch, arr, mom, 0, 0, None), 1),
        ("a null entry", lambda: call(g._h, H(ss[0], None, ss[2]), 3, batch, arr, mom, 0, 0, None), 1),
        ("the same sampler twice", lambda: call(g._h, H(ss[0], ss[1], ss[0]), 3, batch, arr, mom, 0, 0, None), 1),
        ("a sampler of another size", lambda: call(g._h, H(ss[0], ss[1], other), 3, batch, arr, mom, 0, 0, None), 1),
        ("batch not below the data size", lambda: call(g._h, H(*ss), 3, N, arr, mom, 0, 0, None), 1),
        ("validation_size 0", lambda: call(g._h, H(*ss), 3, batch, arr, mom, 0, 0, out), 1),
        ("validation_size N + 1", lambda: call(g._h, H(*ss), 3, batch, arr, mom, 0, N + 1, out), 1),
        ("noise", lambda: call(g._h, H(*ss), 3, batch, arr, mom, 1, 0, None), 3),
    ]
    for what, refused, code in refusals:
        w0 = [m.get_weights() for m in g.members]
        t0 = [m.time for m in g.members]
        assert refused() == code, what
        for k, m in enumerate(g.members):  # nothing was stepped
            assert np.array_equal(m.get_weights(), w0[k]) and m.time == t0[k], what
        # ... nothing drawn, and the group still trains: it stays the twin that was never refused
        g.train_sampled(ss, 3, batch, [0.01, 0.02, 0.03], [0.9, 0.8, 0.7])
        t.train_sampled(st, 3, batch, [0.01, 0.02, 0.03], [0.9, 0.8, 0.7])
        for k in range(K):
            _assert_same(g.members[k], t.members[k], "(after: %s, member %d)" % (what, k))
    for k in range(K):
        assert np.array_equal(ss[k].sample(batch), st[k].sample(batch))
    for bad in (ss[:2], ss + [other], []):
        with pytest.raises(ValueError):
            g.train_sampled(bad, 3, batch, 0.01, 0.9)
        with pytest.raises(ValueError):
            g.train_sampled_observed(bad, 3, batch, 0.01, 0.9, V)
    for x in ss + st + [other, g, t]:
        x.close()


# 10
def test_trainer_with_a_seed_per_member_member_route(gnn, monkeypatch):
    """Member after member (a net off the two-launch path): the observers' text is, line by line, the lone trainers'."""
    N, batch, iters, seeds = 100, 32, 4, [4, 9]
    X, Y = _data(N, OFF_PATH[0], OFF_PATH[-1])
    steps, moms = [0.001, 0.0015], [0.9, 0.85]  # (small: three layers of 1024 on random rows diverge at the other tests' steps)
    g = _group(gnn, monkeypatch, "sce", OFF_PATH, [1, 2], 0, batch)
    assert g.launches_per_step == 0
    tr = gnn.NetGroupTrainer(X, Y, g, seed=seeds)
    streams = [io.StringIO() for _ in seeds]
    tr.train(iters, steps, batch, moms, observers=streams)
    assert g.sampled_each_iterations == (0, iters)
    tr.train(2, steps, batch, moms)  # unobserved, the same entry point
    for k, seed in enumerate(seeds):
        lone = _lone(gnn, monkeypatch, "sce", OFF_PATH, k + 1, 0, batch)
        ltr = gnn.NeuralNetTrainer(X, Y, lone, seed=seed)
        text = io.StringIO()
        ltr.train(iters, steps[k], batch, moms[k], observer=text)
        ltr.train(2, steps[k], batch, moms[k])
        assert streams[k].getvalue().splitlines() == text.getvalue().splitlines() and len(text.getvalue().splitlines()) == iters
        assert np.isfinite(lone.get_weights()).all() and "nan" not in text.getvalue()
        _assert_same(g.members[k], lone, "(member %d)" % k)
        lone.close()
    with pytest.raises(ValueError):
        gnn.NetGroupTrainer(X, Y, g, seed=[1, 2, 3])
    g.close()


def test_trainer_with_a_seed_per_member_grouped_route(gnn, monkeypatch, oracle_mod):
    """Grouped launches.  The observers' text is the formatted curve of the entry point; before formatting that curve agrees
    under close_alpha (1e-12 relative) with the per-iteration form -- a twin group stepped one iteration per call with
    evaluate_range behind each, the form the rule is defined for: fp64 sums of the SAME per-row losses.  The members are bit for
    bit the lone trainers' nets.  The lone trainers' VALUES come from the single-net forward kernel, whose f32 per-row losses
    differ from the grouped validation kernel's in the last bits (2.3e-6 relative at most on an MI355X, printed below), as on the
    shared-sampler route; they are held to the project's budget for a mean loss, 2e-4 |v| + 2e-4 (group_observed_cases.budget)."""
    N, batch, iters, sseeds, _ = fx.FIXTURES["F1"]
    K = len(sseeds)
    X, Y = _data(N, Bn[0], Bn[-1])
    steps, moms = _hyper(K)
    V = N // 100 + 1
    g, twin, p = (_group(gnn, monkeypatch, "sce", Bn, [1, 2, 3], 0, batch) for _ in range(3))
    tr = gnn.NetGroupTrainer(X, Y, g, seed=sseeds)
    assert g.launches_per_step == 2 and len(tr.sampler) == K
    streams = [io.StringIO() for _ in range(K)]
    tr.train(iters, steps, batch, moms, observers=streams)
    assert g.sampled_each_iterations == fx.predict(oracle_mod, "F1")[0]
    for x in (twin, p):
        x.upload_dataset(X, Y)
    ts, ps = _samplers(gnn, "F1"), _samplers(gnn, "F1")
    curve = twin.train_sampled_observed(ts, iters, batch, steps, moms, V)
    ref = []
    for _ in range(iters):
        p.train_sampled(ps, 1, batch, steps, moms)
        ref.append(p.evaluate_range(0, V)[1] / V)
    assert oc.close_alpha(curve, np.array(ref))
    for k in range(K):
        assert streams[k].getvalue() == "".join("%d,%.2f\n" % (i, curve[i, k]) for i in range(iters))
        lone = _lone(gnn, monkeypatch, "sce", Bn, k + 1, 0, batch)
        ltr = gnn.NeuralNetTrainer(X, Y, lone, seed=sseeds[k])
        col = _lone_observed(lone, ltr.sampler, iters, batch, steps[k], moms[k], V)
        print("member", k, "largest relative distance to the lone trainer's values", (np.abs(curve[:, k] - col) / np.abs(col)).max())
        assert (np.abs(curve[:, k] - col) <= oc.budget(col)).all()
        _assert_same(g.members[k], lone, "(member %d)" % k)
        lone.close()
    for x in ts + ps + [g, twin, p]:
        x.close()
