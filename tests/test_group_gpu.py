"""NetGroup (gnn_mlp_group_*): K nets of one shape trained side by side.  Member k after any group call must be bit for bit
the lone handle created with seeds[k] that made the same calls with steps[k], momenta[k] -- weights, momentum and time."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

A = [784, 300, 100, 10]
Bn = [784, 100, 50, 10]


def _data(n, d_in=784, d_out=10, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.random((n, d_in))
    Y = np.eye(d_out)[rng.integers(0, d_out, n)]
    return X, Y


def _hyper(k):
    steps = [0.01 + 0.004 * i for i in range(k)]
    moms = [0.9 - 0.05 * i for i in range(k)]
    return steps, moms


def _lone(gnn, kind, dims, seed, dtype, max_batch):
    if kind == "sce":
        return gnn.SoftmaxCrossEntropyNeuralNet(dims, seed=seed, dtype=dtype, max_batch=max_batch)
    return gnn.GeneralNeuralNet(dims, inner_act="sigmoid", last_act="sigmoid", seed=seed, dtype=dtype, max_batch=max_batch)


def _group(gnn, kind, dims, seeds, dtype, max_batch):
    if kind == "sce":
        return gnn.NetGroup(dims, seeds, dtype=dtype, max_batch=max_batch)
    return gnn.NetGroup(dims, seeds, out_kind=gnn.OUT_ACT_LOSS, inner_act="sigmoid", last_act="sigmoid", dtype=dtype,
                        max_batch=max_batch)


def _assert_same(member, lone, what=""):
    assert np.array_equal(member.get_weights(), lone.get_weights()), "weights differ " + what
    assert np.array_equal(member.get_momentum(), lone.get_momentum()), "momentum differs " + what
    assert member.time == lone.time, "time differs " + what


def _range_case(gnn, kind, dims, K, dtype=0, B=64):
    X, Y = _data(5 * B + 37)  # five batches and a remainder: the row walk wraps
    steps, moms = _hyper(K)
    g = _group(gnn, kind, dims, list(range(1, K + 1)), dtype, B)
    g.upload_dataset(X, Y)
    g.train_range(0, B, 20, steps, moms)
    g.train_range(2 * B, B, 17, steps, moms)
    for k in range(K):
        lone = _lone(gnn, kind, dims, k + 1, dtype, B)
        lone.upload_dataset(X, Y)
        lone.train_range(0, B, 20, steps[k], moms[k])
        lone.train_range(2 * B, B, 17, steps[k], moms[k])
        _assert_same(g.members[k], lone, "(member %d)" % k)
        lone.close()
    return g


@pytest.mark.parametrize("K", [1, 3, 8])
def test_train_range_matches_lone_handles(gnn, K):
    g = _range_case(gnn, "sce", A, K)
    assert g.launches_per_step == 2
    assert g.members[0].rowblock_state == 2  # the prebuilt static instance
    g.close()


@pytest.mark.parametrize("kind,dims,dtype", [
    ("sce", Bn, 0),
    ("sce", A, 1),
    ("gnn", A, 0),
], ids=["784-100-50-10-f32", "784-300-100-10-bf16", "general-sigmoid-f32"])
def test_train_range_other_nets(gnn, kind, dims, dtype):
    g = _range_case(gnn, kind, dims, 3, dtype)
    assert g.launches_per_step == 2
    g.close()


def test_train_range_runtime_shape(gnn):
    dims = [784, 200, 64, 10]  # not prebuilt: the runtime-shape grouped instance
    probe = gnn.SoftmaxCrossEntropyNeuralNet(dims, max_batch=64)
    assert probe.step_launches == 2 and probe.rowblock_state == 1
    probe.close()
    g = _range_case(gnn, "sce", dims, 3)
    assert g.launches_per_step == 2
    g.close()


@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
def test_train_sampled_shared_sampler(gnn, dtype):
    N, batch, iters, K = 1000, 96, 25, 3  # 2 400 draws: epoch boundaries, batches shortened at a refill
    X, Y = _data(N, seed=3)
    steps, moms = _hyper(K)
    g = gnn.NetGroup(A, [1, 2, 3], dtype=dtype, max_batch=batch)
    g.upload_dataset(X, Y)
    s = gnn.Sampler(N, seed=1)
    g.train_sampled(s, iters, batch, steps, moms)
    g.train_sampled(s, 7, batch, steps, moms)
    for k in range(K):
        lone = gnn.SoftmaxCrossEntropyNeuralNet(A, seed=k + 1, dtype=dtype, max_batch=batch)
        lone.upload_dataset(X, Y)
        ls = gnn.Sampler(N, seed=1)
        for n in (iters, 7):
            C_ = lone._lib.gnn_mlp_train_sampled(lone._h, ls._h, n, batch, steps[k], moms[k], 0)
            assert C_ == 0
        _assert_same(g.members[k], lone, "(member %d)" % k)
        lone.close()
        ls.close()
    # the shared sampler ends where one lone sampler ends
    ref = gnn.Sampler(N, seed=1)
    for _ in range(iters + 7):
        ref.sample(batch)
    assert np.array_equal(s.sample(batch), ref.sample(batch))
    g.close()


def test_fallback_off_the_two_launch_path(gnn):
    dims = [784, 1024, 1024, 1024, 10]
    probe = gnn.SoftmaxCrossEntropyNeuralNet(dims, max_batch=32)
    assert probe.step_launches != 2
    probe.close()
    X, Y = _data(100)
    steps, moms = _hyper(2)
    g = gnn.NetGroup(dims, [1, 2], max_batch=32)
    assert g.launches_per_step == 0
    g.upload_dataset(X, Y)
    g.train_range(0, 32, 4, steps, moms)
    for k in range(2):
        lone = gnn.SoftmaxCrossEntropyNeuralNet(dims, seed=k + 1, max_batch=32)
        lone.upload_dataset(X, Y)
        lone.train_range(0, 32, 4, steps[k], moms[k])
        _assert_same(g.members[k], lone, "(member %d)" % k)
        lone.close()
    g.close()


def test_members_are_full_handles(gnn, tmp_path):
    B, K = 64, 3
    X, Y = _data(5 * B + 11, seed=5)
    steps, moms = _hyper(K)
    g = gnn.NetGroup(A, [1, 2, 3], max_batch=B)
    g.upload_dataset(X, Y)
    g.train_range(0, B, 9, steps, moms)
    lones = []
    for k in range(K):
        lone = gnn.SoftmaxCrossEntropyNeuralNet(A, seed=k + 1, max_batch=B)
        lone.upload_dataset(X, Y)
        lone.train_range(0, B, 9, steps[k], moms[k])
        lones.append(lone)
    m, lone = g.members[1], lones[1]
    _assert_same(m, lone)
    Xq, Yq = X[:B], Y[:B]
    assert np.array_equal(m.propagate(Xq), lone.propagate(Xq))
    assert np.array_equal(m.calculateLoss(Xq, Yq), lone.calculateLoss(Xq, Yq))
    assert np.array_equal(m.argmax(Xq), lone.argmax(Xq))
    assert m.count_hits_range() == lone.count_hits_range()
    # checkpoint round trip: out of a member, into a fresh net, and back into the member
    path = tmp_path / "member1.ckpt"
    m.save_checkpoint(path)
    fresh = gnn.SoftmaxCrossEntropyNeuralNet(A, seed=99, max_batch=B)
    fresh.load_checkpoint(path)
    _assert_same(fresh, m, "(checkpoint)")
    m.load_checkpoint(path)
    _assert_same(m, lone, "(after loading its own checkpoint)")
    fresh.close()
    # a lone step on one member (its update deferred into the next call), then more group training
    Xs, Ys = _data(B, seed=9)
    m.gradientStep(Xs, 0.02, 0.8, False, expected=Ys)
    lone.gradientStep(Xs, 0.02, 0.8, False, expected=Ys)
    g.train_range(3 * B, B, 6, steps, moms)
    for k in range(K):
        lones[k].train_range(3 * B, B, 6, steps[k], moms[k])
        _assert_same(g.members[k], lones[k], "(member %d after a lone step)" % k)
        lones[k].close()
    g.close()


def test_refusals(gnn):
    lib = gnn.load_library()
    for K in (0, 17):
        with pytest.raises(gnn.GnnError) as e:
            gnn.NetGroup(A, list(range(1, K + 1)), max_batch=64)
        assert e.value.code == 1
    X, Y = _data(300)
    g = gnn.NetGroup(A, [1, 2], max_batch=64)
    g.upload_dataset(X, Y)
    with pytest.raises(ValueError):
        g.train_range(0, 64, 2, [0.01, 0.02, 0.03], 0.9)
    with pytest.raises(ValueError):
        g.train_range(0, 64, 2, 0.01, [0.9])
    st = (C.c_double * 2)(0.01, 0.02)
    assert lib.gnn_mlp_group_train_range(g._h, 0, 64, 2, None, st) == 1
    assert lib.gnn_mlp_group_train_range(g._h, 0, 64, 2, st, None) == 1
    s = gnn.Sampler(300, seed=1)
    with pytest.raises(gnn.GnnError) as e:
        g.train_sampled(s, 3, 32, 0.01, 0.9, noise=True)
    assert e.value.code == 3
    with pytest.raises(gnn.GnnError) as e:
        g.train_range(0, 128, 2, 0.01, 0.9)  # B above max_batch
    assert e.value.code == 1
    with pytest.raises(gnn.GnnError) as e:
        g.train_range(32, 64, 2, 0.01, 0.9)  # first not a multiple of B
    assert e.value.code == 1
    h = C.c_void_p()
    assert lib.gnn_mlp_group_member(g._h, 2, C.byref(h)) == 1
    assert lib.gnn_mlp_group_member(g._h, -1, C.byref(h)) == 1
    m = g.members[0]
    assert lib.gnn_mlp_destroy(m._h) == 5
    with pytest.raises(gnn.GnnError) as e:
        m.upload_dataset(X, Y)
    assert e.value.code == 5
    with pytest.raises(gnn.GnnError) as e:
        m.set_stream(None)
    assert e.value.code == 5
    # the refused destroy freed nothing: the members still train, alone and in the group
    w0 = m.get_weights()
    m.gradientStep(X[:64], 0.01, 0.9, False, expected=Y[:64])
    g.train_range(0, 64, 3, 0.01, 0.9)
    assert not np.array_equal(m.get_weights(), w0)
    assert m.time == 4 and g.members[1].time == 3
    s.close()
    g.close()
