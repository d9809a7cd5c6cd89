"""A NetGroup trained with ONE BATCH SIZE PER MEMBER (gnn_mlp_group_train_sampled_sizes; NetGroup.train_sampled([s_0 .. s_{K-1}], ..,
batch=[b_0 .. b_{K-1}], ..)) -- the reference's recorded sweep, logs/trainLog.csv rows 1-3, as one call.

The one rule: member k is, bit for bit (weights, momentum, time), the lone net created with seeds[k] after gnn_mlp_train_sampled
with a fresh sampler of s_k's seed and batches[k]; every s_k's next draw is the lone run's sampler's next draw; and
NetGroup.sampled_each_iterations says (iterations, 0) on a group with grouped launches -- EVERY iteration is the two grouped
launches, member k with its own live row count -- and (0, iterations) on one without.  Every comparison is bitwise, against lone
nets driven through the existing ABI (which other tests hold to the fp64 oracles).  The fixtures: tests/group_batch_cases.py;
what they contain (different pads, one and two TS_KC chunks, a single row, batches a refill shortened for one member only):
tests/test_group_batches_cpu.py."""
import ctypes as C

import numpy as np
import pytest

from tests import chain_cases as cc
from tests import group_batch_cases as bc
from tests import static_instance_cases as sc
from tests import test_group_samplers_cpu as fx

pytestmark = pytest.mark.gpu

Bn = [784, 100, 50, 10]       # prebuilt instances
SMALL = [65, 20, 12, 5]       # runtime-shape instances, one ragged 4-row block
OFF_PATH = [784, 1024, 1024, 1024, 10]
CHAIN_SEED = 18               # tests/chain_cases.py: 890-166-78-15, a ragged input width (13 slabs and 58 inputs), f32 and bf16 forms
# tests/group_batch_cases.py's, and the samplers of tests/test_group_samplers_cpu.py's F5 drawing one size per member: 260
# iterations, five sampler chunks of the loop, a batch shortened for one member only in every one of them
FIXTURES = dict(bc.FIXTURES, F5=(fx.FIXTURES["F5"][0], list(fx.F5_SIZES), fx.FIXTURES["F5"][2], fx.FIXTURES["F5"][3], [1, 2, 3]))


def _lone(gnn, monkeypatch, kind, dims, seed, dtype, max_batch, inner=None):
    with monkeypatch.context() as m:
        m.setenv("GNN_MLP_JIT", "0")
        if kind == "sce":
            kw = {} if inner is None else {"inner_act": inner}
            return gnn.SoftmaxCrossEntropyNeuralNet(dims, seed=seed, dtype=dtype, max_batch=max_batch, **kw)
        return gnn.GeneralNeuralNet(dims, inner_act="sigmoid", last_act="sigmoid", seed=seed, dtype=dtype, max_batch=max_batch)


def _group(gnn, monkeypatch, kind, dims, seeds, dtype, max_batch, inner=None):
    with monkeypatch.context() as m:
        m.setenv("GNN_MLP_JIT", "0")
        if kind == "sce":
            kw = {} if inner is None else {"inner_act": inner}
            return gnn.NetGroup(dims, seeds, dtype=dtype, max_batch=max_batch, **kw)
        return gnn.NetGroup(dims, seeds, out_kind=gnn.OUT_ACT_LOSS, inner_act="sigmoid", last_act="sigmoid", dtype=dtype,
                            max_batch=max_batch)


def _assert_same(member, lone, what=""):
    w = member.get_weights()
    assert np.isfinite(w).all(), "weights not finite " + what
    assert np.array_equal(w, lone.get_weights()), "weights differ " + what
    assert np.array_equal(member.get_momentum(), lone.get_momentum()), "momentum differs " + what
    assert member.time == lone.time, "time differs " + what


def _lone_sampled(lone, s, n, batch, step, mom):
    assert lone._lib.gnn_mlp_train_sampled(lone._h, s._h, n, batch, step, mom, 0) == 0


def _lone_observed(lone, s, n, batch, step, mom, V):
    val = np.empty(n)
    rc = lone._lib.gnn_mlp_train_sampled_observed(lone._h, s._h, n, batch, step, mom, 0, V, val.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == 0
    return val


def _one_rule(gnn, monkeypatch, name, kind, dims, dtype, calls=None, steps=None, moms=None, max_batch=None, inner=None, w_scale=None,
              expect_grouped=True):
    N, batches, iters, sseeds, wseeds = FIXTURES[name]
    calls = [iters] if calls is None else calls
    K = len(batches)
    max_batch = max(batches) if max_batch is None else max_batch
    X, Y = bc.data(N, dims[0], dims[-1])
    if steps is None:
        steps, moms = bc.hyper(K)
    g = _group(gnn, monkeypatch, kind, dims, wseeds, dtype, max_batch, inner)
    assert g.launches_per_step == (2 if expect_grouped else 0)
    if w_scale is not None:
        for m in g.members:
            m.set_weights(m.get_weights() * w_scale)
    g.upload_dataset(X, Y)
    ss = [gnn.Sampler(N, seed=s) for s in sseeds]
    for n in calls:
        g.train_sampled(ss, n, batches, steps, moms)
        assert g.sampled_each_iterations == ((n, 0) if expect_grouped and K > 1 else (0, n)), (name, n)
    ls = [gnn.Sampler(N, seed=s) for s in sseeds]
    for k in range(K):
        lone = _lone(gnn, monkeypatch, kind, dims, wseeds[k], dtype, max_batch, inner)
        if w_scale is not None:
            lone.set_weights(lone.get_weights() * w_scale)
        lone.upload_dataset(X, Y)
        for n in calls:
            _lone_sampled(lone, ls[k], n, batches[k], steps[k], moms[k])
        _assert_same(g.members[k], lone, "(%s member %d, batch %d)" % (name, k, batches[k]))
        assert np.array_equal(ss[k].sample(batches[k]), ls[k].sample(batches[k])), "sampler %d ends elsewhere" % k
        lone.close()
    for x in ss + ls + [g]:
        x.close()


# 1 -- the reference's recorded sweep
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
def test_prebuilt_shape_the_recorded_sweep_two_calls(gnn, monkeypatch, dtype):
    _one_rule(gnn, monkeypatch, "SWEEP", "sce", Bn, dtype, calls=bc.SWEEP_CALLS, steps=bc.SWEEP_STEPS, moms=[bc.SWEEP_MOMENTUM] * 3)


# 2 -- runtime-shape instances, two 16-row pads, a single row
@pytest.mark.parametrize("kind,dtype", [("sce", 0), ("sce", 1), ("gnn", 0)], ids=["sce-f32", "sce-bf16", "general-f32"])
def test_runtime_shape_ragged_batches(gnn, monkeypatch, kind, dtype):
    _one_rule(gnn, monkeypatch, "RAGGED", kind, SMALL, dtype)


# 3 -- one launch holds members of one and of two TS_KC chunks, on the full-chunk paths and on the guarded ones
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("net", ["chain-case", "small"])
def test_two_chunks_beside_one(gnn, monkeypatch, net, dtype):
    if net == "small":
        _one_rule(gnn, monkeypatch, "CHUNKS", "sce", SMALL, dtype, max_batch=144)
        return
    dims, _, inner, out_kind, _ = cc.chain_case(CHAIN_SEED)
    assert out_kind == cc.OUT_SOFTMAX_CE and dims[0] % 64 != 0 and len(dims) == 4
    K = len(bc.FIXTURES["CHUNKS"][1])
    _one_rule(gnn, monkeypatch, "CHUNKS", "sce", dims, dtype, max_batch=144, inner=inner, w_scale=cc.W_SCALE,
              steps=[cc.STEP * (1 + k / 32) for k in range(K)], moms=[cc.MOMENTUM - 0.01 * k for k in range(K)])


# 4 -- the whole GroupArgs arrays
def test_sixteen_members_batches_1_to_16(gnn, monkeypatch):
    _one_rule(gnn, monkeypatch, "SIXTEEN", "sce", SMALL, 0)


# 4b -- member offsets across the loop's sampler chunks (they begin at iterations 0, 16, 48, 112, 240) and the wrap of its ring of four slots
def test_across_chunk_boundaries_and_the_rings_wrap(gnn, monkeypatch):
    _one_rule(gnn, monkeypatch, "F5", "sce", SMALL, 0)  # (asserts sampled_each_iterations == (260, 0): every iteration grouped)


# 5 -- the observed form
@pytest.mark.parametrize("name,dims", [("SWEEP", Bn), ("RAGGED", SMALL)], ids=["prebuilt", "runtime-shape"])
def test_observed_columns_are_the_lone_curves(gnn, monkeypatch, name, dims):
    """Column k of the curve equals the lone handle's gnn_mlp_train_sampled_observed curve bit for bit; the members and samplers
    end as after the unobserved call."""
    N, batches, iters, sseeds, wseeds = bc.FIXTURES[name]
    K, V = len(batches), 3
    X, Y = bc.data(N, dims[0], dims[-1])
    steps, moms = bc.hyper(K)
    g, t = (_group(gnn, monkeypatch, "sce", dims, wseeds, 0, max(batches)) for _ in range(2))
    for x in (g, t):
        x.upload_dataset(X, Y)
    assert g.launches_per_step == 2 and g.observed_launches == 3
    sg, st, ls = ([gnn.Sampler(N, seed=s) for s in sseeds] for _ in range(3))
    curve = g.train_sampled_observed(sg, iters, batches, steps, moms, V)
    assert curve.shape == (iters, K) and g.sampled_each_iterations == (iters, 0)
    t.train_sampled(st, iters, batches, steps, moms)
    worst = 0.0
    cols = []
    for k in range(K):
        _assert_same(g.members[k], t.members[k], "(observed against unobserved, member %d)" % k)
        assert np.array_equal(sg[k].sample(batches[k]), st[k].sample(batches[k]))
        lone = _lone(gnn, monkeypatch, "sce", dims, wseeds[k], 0, max(batches))
        lone.upload_dataset(X, Y)
        cols.append(_lone_observed(lone, ls[k], iters, batches[k], steps[k], moms[k], V))
        _assert_same(g.members[k], lone, "(member %d)" % k)
        worst = max(worst, float((np.abs(curve[:, k] - cols[k]) / np.abs(cols[k])).max()))
        lone.close()
    print(name, "largest relative distance between a column and the lone curve:", worst)
    for k in range(K):
        assert np.array_equal(curve[:, k], cols[k]), "column %d is not the lone curve (largest relative distance %g)" % (k, worst)
    for x in sg + st + ls + [g, t]:
        x.close()


# 6 -- equal batches through the new entry: the end state of _each, no iteration member after member
@pytest.mark.parametrize("name,dims", [("F1", Bn), ("F2", SMALL)])
def test_equal_batches_every_iteration_grouped(gnn, monkeypatch, oracle_mod, name, dims):
    N, batch, iters, sseeds, _ = fx.FIXTURES[name]
    K = len(sseeds)
    X, Y = bc.data(N, dims[0], dims[-1])
    steps, moms = bc.hyper(K)
    a, b = (_group(gnn, monkeypatch, "sce", dims, [1, 2, 3], 0, batch) for _ in range(2))
    for x in (a, b):
        x.upload_dataset(X, Y)
    sa, sb = ([gnn.Sampler(N, seed=s) for s in sseeds] for _ in range(2))
    a.train_sampled(sa, iters, batch, steps, moms)            # gnn_mlp_group_train_sampled_each
    (grouped, mixed), _ = fx.predict(oracle_mod, name)
    assert a.sampled_each_iterations == (grouped, mixed) and mixed > 0
    b.train_sampled(sb, iters, [batch] * K, steps, moms)      # gnn_mlp_group_train_sampled_sizes
    assert b.sampled_each_iterations == (iters, 0)
    for k in range(K):
        _assert_same(b.members[k], a.members[k], "(%s member %d)" % (name, k))
        assert np.array_equal(sa[k].sample(batch), sb[k].sample(batch))
    for x in sa + sb + [a, b]:
        x.close()


# 7 -- off the grouped path: member after member with batches[k]
@pytest.mark.parametrize("which", ["off-the-two-launch-path", "one-member", "rowblock-off"])
def test_off_the_grouped_path(gnn, monkeypatch, which):
    if which == "rowblock-off":
        monkeypatch.setenv("GNN_MLP_ROWBLOCK", "0")
    dims = OFF_PATH if which == "off-the-two-launch-path" else SMALL
    batches = [7] if which == "one-member" else [5, 12] if which == "off-the-two-launch-path" else [1, 12, 9]
    steps = [0.001, 0.0015, 0.002] if which == "off-the-two-launch-path" else [0.01, 0.014, 0.018]
    K, N, iters, V = len(batches), 29, 9, 3
    X, Y = bc.data(N, dims[0], dims[-1])
    moms = [0.9, 0.85, 0.8][:K]
    g, o = (_group(gnn, monkeypatch, "sce", dims, list(range(1, K + 1)), 0, max(batches)) for _ in range(2))
    assert g.launches_per_step == (2 if which == "one-member" else 0)
    for x in (g, o):
        x.upload_dataset(X, Y)
    ss, so, ls, lo = ([gnn.Sampler(N, seed=k + 1) for k in range(K)] for _ in range(4))
    g.train_sampled(ss, iters, batches, steps[:K], moms)
    assert g.sampled_each_iterations == (0, iters)
    curve = o.train_sampled_observed(so, iters, batches, steps[:K], moms, V)
    assert o.sampled_each_iterations == (0, iters) and curve.shape == (iters, K)
    for k in range(K):
        lone, lobs = (_lone(gnn, monkeypatch, "sce", dims, k + 1, 0, max(batches)) for _ in range(2))
        for x in (lone, lobs):
            x.upload_dataset(X, Y)
        _lone_sampled(lone, ls[k], iters, batches[k], steps[k], moms[k])
        col = _lone_observed(lobs, lo[k], iters, batches[k], steps[k], moms[k], V)
        _assert_same(g.members[k], lone, "(member %d)" % k)
        _assert_same(o.members[k], lobs, "(observed, member %d)" % k)
        assert np.array_equal(curve[:, k], col)
        assert np.array_equal(ss[k].sample(batches[k]), ls[k].sample(batches[k])) and np.array_equal(so[k].sample(batches[k]), lo[k].sample(batches[k]))
        for x in (lone, lobs):
            x.close()
    for x in ss + so + ls + lo + [g, o]:
        x.close()


# 8 -- between the other group calls and a member stepped alone (enter_grouped with per-member look-ahead sizes)
def test_interleaved_with_the_other_calls(gnn, monkeypatch):
    N, batches, _, sseeds, wseeds = bc.FIXTURES["RAGGED"]
    K, B = len(batches), 12
    X, Y = bc.data(N, SMALL[0], SMALL[-1])
    steps, moms = bc.hyper(K)
    g = _group(gnn, monkeypatch, "sce", SMALL, wseeds, 0, max(batches))
    g.upload_dataset(X, Y)
    ss = [gnn.Sampler(N, seed=s) for s in sseeds]
    g.train_sampled(ss, 6, batches, steps, moms)
    assert g.sampled_each_iterations == (6, 0)
    g.train_sampled(ss, 3, batches, steps, moms)            # straight after: the members' states are found as they were left
    g.train_range(0, B, 3, steps, moms)
    g.members[2].gradient_step_range(3, B, 0.02, 0.8)       # one member alone
    g.train_sampled(ss, 5, batches, steps, moms)
    assert g.sampled_each_iterations == (5, 0)
    g.members[0].gradient_step_range(5, 7, 0.02, 0.8)       # member 0 alone, another size: its state is its own again
    g.train_sampled(ss, 4, batches, steps, moms)
    g.train_range(B, B, 2, steps, moms)
    ls = [gnn.Sampler(N, seed=s) for s in sseeds]
    for k in range(K):
        lone = _lone(gnn, monkeypatch, "sce", SMALL, wseeds[k], 0, max(batches))
        lone.upload_dataset(X, Y)
        _lone_sampled(lone, ls[k], 6, batches[k], steps[k], moms[k])
        _lone_sampled(lone, ls[k], 3, batches[k], steps[k], moms[k])
        lone.train_range(0, B, 3, steps[k], moms[k])
        if k == 2:
            lone.gradient_step_range(3, B, 0.02, 0.8)
        _lone_sampled(lone, ls[k], 5, batches[k], steps[k], moms[k])
        if k == 0:
            lone.gradient_step_range(5, 7, 0.02, 0.8)
        _lone_sampled(lone, ls[k], 4, batches[k], steps[k], moms[k])
        lone.train_range(B, B, 2, steps[k], moms[k])
        _assert_same(g.members[k], lone, "(member %d)" % k)
        assert np.array_equal(ss[k].sample(batches[k]), ls[k].sample(batches[k]))
        lone.close()
    for x in ss + ls + [g]:
        x.close()


# 9 -- refusals: before any draw and any step
def test_refusals(gnn, monkeypatch):
    lib = gnn.load_library()
    N, K, V, max_batch = 40, 3, 3, 12
    good = [5, 12, 8]
    X, Y = bc.data(N, SMALL[0], SMALL[-1])
    g, t = (_group(gnn, monkeypatch, "sce", SMALL, [1, 2, 3], 0, max_batch) for _ in range(2))
    for x in (g, t):
        x.upload_dataset(X, Y)
    ss, st = ([gnn.Sampler(N, seed=k + 1) for k in range(K)] for _ in range(2))
    other = gnn.Sampler(N + 1, seed=1)
    arr, mom = (C.c_double * K)(0.01, 0.02, 0.03), (C.c_double * K)(0.9, 0.8, 0.7)
    val = np.empty((3, K))
    out = val.ctypes.data_as(C.POINTER(C.c_double))
    H = lambda *s: (C.c_void_p * K)(*[x._h if x is not None else None for x in s])
    I = lambda *b: (C.c_int32 * K)(*b)
    call = lib.gnn_mlp_group_train_sampled_sizes
    BAD_ARG, UNSUPPORTED = 1, 3
    refusals = [
        ("null batches", lambda: call(g._h, H(*ss), 3, None, arr, mom, 0, 0, None), BAD_ARG),
        ("a batch of 0", lambda: call(g._h, H(*ss), 3, I(5, 0, 8), arr, mom, 0, 0, None), BAD_ARG),
        ("a negative batch", lambda: call(g._h, H(*ss), 3, I(5, 12, -1), arr, mom, 0, 0, None), BAD_ARG),
        ("a batch above max_batch", lambda: call(g._h, H(*ss), 3, I(5, max_batch + 1, 8), arr, mom, 0, 0, None), BAD_ARG),
        ("null samplers", lambda: call(g._h, None, 3, I(*good), arr, mom, 0, 0, None), BAD_ARG),
        ("a null entry", lambda: call(g._h, H(ss[0], None, ss[2]), 3, I(*good), arr, mom, 0, 0, None), BAD_ARG),
        ("the same sampler twice", lambda: call(g._h, H(ss[0], ss[1], ss[0]), 3, I(*good), arr, mom, 0, 0, None), BAD_ARG),
        ("a sampler of another size", lambda: call(g._h, H(ss[0], ss[1], other), 3, I(*good), arr, mom, 0, 0, None), BAD_ARG),
        ("iterations 0", lambda: call(g._h, H(*ss), 0, I(*good), arr, mom, 0, 0, None), BAD_ARG),
        ("validation_size 0", lambda: call(g._h, H(*ss), 3, I(*good), arr, mom, 0, 0, out), BAD_ARG),
        ("validation_size N + 1", lambda: call(g._h, H(*ss), 3, I(*good), arr, mom, 0, N + 1, out), BAD_ARG),
        ("noise", lambda: call(g._h, H(*ss), 3, I(*good), arr, mom, 1, 0, None), UNSUPPORTED),
    ]
    for what, refused, code in refusals:
        w0 = [m.get_weights() for m in g.members]
        t0 = [m.time for m in g.members]
        assert refused() == code, what
        for k, m in enumerate(g.members):  # nothing was stepped
            assert np.array_equal(m.get_weights(), w0[k]) and m.time == t0[k], what
        # ... nothing drawn, and the group still trains: it stays the twin that was never refused
        g.train_sampled(ss, 3, good, [0.01, 0.02, 0.03], [0.9, 0.8, 0.7])
        t.train_sampled(st, 3, good, [0.01, 0.02, 0.03], [0.9, 0.8, 0.7])
        for k in range(K):
            _assert_same(g.members[k], t.members[k], "(after: %s, member %d)" % (what, k))
    for k in range(K):
        assert np.array_equal(ss[k].sample(good[k]), st[k].sample(good[k]))
    # a batch not below the data set's rows (NNT:63): a group whose max_batch admits it
    big = _group(gnn, monkeypatch, "sce", SMALL, [1, 2, 3], 0, N)
    big.upload_dataset(X, Y)
    w0 = [m.get_weights() for m in big.members]
    assert call(big._h, H(*ss), 3, I(5, N, 8), arr, mom, 0, 0, None) == BAD_ARG
    for k, m in enumerate(big.members):
        assert np.array_equal(m.get_weights(), w0[k]) and m.time == 0
    for k in range(K):
        assert np.array_equal(ss[k].sample(good[k]), st[k].sample(good[k]))
    # Python: a batch sequence needs a sampler per member, and one size per member
    one = gnn.Sampler(N, seed=9)
    for sampler, batch in ((one, good), (ss, good[:2]), (ss, good + [3])):
        with pytest.raises(ValueError):
            g.train_sampled(sampler, 3, batch, 0.01, 0.9)
        with pytest.raises(ValueError):
            g.train_sampled_observed(sampler, 3, batch, 0.01, 0.9, V)
    for k, m in enumerate(g.members):
        assert m.time == t.members[k].time
    for x in ss + st + [other, one, g, t, big]:
        x.close()


# 10 -- every entry of the prebuilt tables of the SIZED row-block instances (csrc/static_shapes.h asked for RbGroupSized)
@pytest.mark.parametrize("bf", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["softmax", "general"])
@pytest.mark.parametrize("inner", range(5), ids=sc.ACT_IDS)
@pytest.mark.parametrize("dims", sc.SHAPES, ids=["784-300-100-10", "784-100-50-10"])
def test_sized_prebuilt_instance(gnn, monkeypatch, dims, inner, kind, bf):
    """Two members with batches 3 and 6 (one and two 4-row blocks) over five iterations of a 12-row data set, bit for bit the lone
    nets -- which tests/test_static_instances_gpu.py holds to the fp64 oracle per activation: a wrong table entry is a kernel built
    for another activation or output rule, and tests/test_static_instances_cpu.py puts those outside the budgets, far from equal."""
    monkeypatch.setenv("GNN_MLP_JIT", "0")
    dtype = gnn.DTYPE_BF16 if bf else gnn.DTYPE_F32
    X, Y = sc.dataset(dims[0], dims[-1])
    N, batches, iters = X.shape[0], [3, 6], 5
    kw = dict(inner_act=inner, dtype=dtype, max_batch=sc.B)
    if kind == "general":
        g = gnn.NetGroup(dims, [1, 2], out_kind=gnn.OUT_ACT_LOSS, last_act=sc.LAST, **kw)
    else:
        g = gnn.NetGroup(dims, [1, 2], **kw)
    assert g.launches_per_step == 2 and g.members[0].specialization == 1
    for m in g.members:
        m.set_weights(m.get_weights() * sc.SCALE[inner])
    g.upload_dataset(X, Y)
    ss, ls = ([gnn.Sampler(N, seed=k + 1) for k in range(2)] for _ in range(2))
    g.train_sampled(ss, iters, batches, [h[0] for h in sc.HYPER], [h[1] for h in sc.HYPER])
    assert g.sampled_each_iterations == (iters, 0)
    for k in range(2):
        if kind == "general":
            lone = gnn.GeneralNeuralNet(dims, last_act=sc.LAST, seed=k + 1, **kw)
        else:
            lone = gnn.SoftmaxCrossEntropyNeuralNet(dims, seed=k + 1, **kw)
        lone.set_weights(lone.get_weights() * sc.SCALE[inner])
        lone.upload_dataset(X, Y)
        _lone_sampled(lone, ls[k], iters, batches[k], *sc.HYPER[k])
        _assert_same(g.members[k], lone, "(member %d)" % k)
        lone.close()
    for x in ss + ls + [g]:
        x.close()


# 11 -- NetGroupTrainer with a sequence as batchSize
def test_trainer_with_a_batch_size_per_member(gnn, monkeypatch):
    N, batches, iters, sseeds, wseeds = bc.FIXTURES["RAGGED"]
    K = len(batches)
    X, Y = bc.data(N, SMALL[0], SMALL[-1])
    steps, moms = bc.hyper(K)
    g = _group(gnn, monkeypatch, "sce", SMALL, wseeds, 0, max(batches))
    tr = gnn.NetGroupTrainer(X, Y, g, seed=sseeds)
    tr.train(iters, steps, batches, moms)
    assert g.sampled_each_iterations == (iters, 0)
    for k in range(K):
        lone = _lone(gnn, monkeypatch, "sce", SMALL, wseeds[k], 0, max(batches))
        ltr = gnn.NeuralNetTrainer(X, Y, lone, seed=sseeds[k])
        ltr.train(iters, steps[k], batches[k], moms[k])
        _assert_same(g.members[k], lone, "(member %d)" % k)
        lone.close()
    with pytest.raises(ValueError):
        tr.train(iters, steps, batches[:2], moms)
    with pytest.raises(ValueError):
        tr.train(iters, steps, [1, 16, N, 12], moms)
    shared = gnn.NetGroupTrainer(X, Y, g, seed=1)   # one sampler for all: a batch sequence cannot be served
    with pytest.raises(ValueError):
        shared.train(iters, steps, batches, moms)
    g.close()
