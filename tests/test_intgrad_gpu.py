"""Integrated gradients on the device (gnn_mlp_integrated_gradients_set_range; csrc/input_grad.hip, csrc/input_grad_kernel.h:
intgrad_kernel, intgrad_start_kernel, intgrad_delta_kernel) on the fixtures of tests/intgrad_cases.py.

Against the fp64 model: every live cell of every fixture within the element budget (f32, and bf16 on the four bf16 fixtures); no
cell is excluded.  Exact twins (bit for bit): gnn_amd.integrated_gradients, the host route over the same blocks; the maps and
class counts against numpy on the returned attributions; a sub-range on a block boundary, a repeated call, the held-out set
against a net that holds those rows as its training set, input_gradient_range around a call, and "nothing moves" in training.
Completeness: |delta| within the model's own recorded gap + the row's element budgets + the loss budget of the two losses, and
delta against gnn_amd.convergence_delta to the order of an fp64 sum."""
import ctypes as C

import numpy as np
import pytest

from tests import adversarial_cases as ac
from tests import intgrad_cases as ic

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1
TWINS = [(name, BF16 if bf else F32) for name, bf in ic.ALL]
M = ic.STEPS


def make_net(gnn, oracle_mod, c, dtype=F32, max_batch=None):
    net = gnn.SoftmaxCrossEntropyNeuralNet(c.dims, inner_act=c.inner, seed=1, dtype=dtype, max_batch=max_batch or c.max_batch)
    net.set_weights(ac.flat_weights(oracle_mod, c))
    return net


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def expected_rule(Y):
    """MT:186-188: the LAST index whose expected value is exactly 1, 0 when there is none."""
    return np.array([int(np.flatnonzero(r == 1.0)[-1]) if (r == 1.0).any() else 0 for r in np.asarray(Y)], dtype=np.int64)


def host_route(gnn, net, X, Y, first, n, max_batch, steps=M, baseline=0.0):
    """gnn_amd.integrated_gradients over the blocks of max_batch rows the range call takes"""
    out = []
    for off in range(first, first + n, max_batch):
        rows = slice(off, min(off + max_batch, first + n))
        out.append(gnn.integrated_gradients(net, X[rows], Y[rows], steps, baseline))
    return np.concatenate(out)


def block_losses(net, X, Y, mb):
    return np.concatenate([np.atleast_1d(net.calculateLoss(X[o:o + mb], Y[o:o + mb])) for o in range(0, len(X), mb)])


# ---- 1. the model -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", TWINS)
def test_every_live_cell_is_within_the_budget(gnn, oracle_mod, name, dtype):
    c = ac.BY_NAME[name]
    bf = dtype == BF16
    X, Y = ac.rows(c)
    net = make_net(gnn, oracle_mod, c, dtype)
    net.upload_dataset(X, Y)
    runs = [(M, b) for b in ic.BASELINES] + ([ic.ONE_STEP[1:]] if name == ic.ONE_STEP[0] else [])
    for steps, baseline in runs:
        ref = ic.reference(oracle_mod, c, baseline, bf, steps)
        ig = net.integrated_gradients_range(steps, baseline)
        assert ig.shape == X.shape and ig.dtype == np.float64
        err = np.abs(ig - ref.ig)
        worst = float((err / np.where(ref.budget > 0, ref.budget, 1.0)).max())
        print("%s %s steps %d b=%.2f: worst cell %.3g budgets, max|IG| %.3g" % (name, "bf16" if bf else "f32", steps, baseline, worst, np.abs(ref.ig).max()))
        assert np.all(err <= ref.budget)
        assert np.all(ig[np.asarray(ref.d) == 0] == 0)


# ---- 2. the host route, bit for bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", TWINS)
def test_attributions_are_the_host_route(gnn, oracle_mod, name, dtype):
    c = ac.BY_NAME[name]
    X, Y = ac.rows(c)
    net = make_net(gnn, oracle_mod, c, dtype)
    net.upload_dataset(X, Y)
    runs = [(M, b) for b in ic.BASELINES] + ([ic.ONE_STEP[1:]] if name == ic.ONE_STEP[0] else [])
    for steps, baseline in runs:
        ig = net.integrated_gradients_range(steps, baseline)
        want = host_route(gnn, net, X, Y, 0, c.n, c.max_batch, steps, baseline)
        assert same_bits(ig, want), (name, steps, baseline, int((ig != want).sum()))
        assert np.array_equal(ig, want)                       # (the fp64 values are the f32 values widened)
    if c.n > 8:                                               # a range that starts inside the set
        got = net.integrated_gradients_range(M, 0.25, 3, c.n - 5)
        assert same_bits(got, host_route(gnn, net, X, Y, 3, c.n - 5, c.max_batch, M, 0.25))


# ---- 3. completeness ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", TWINS)
def test_completeness_on_the_device(gnn, oracle_mod, name, dtype):
    c = ac.BY_NAME[name]
    X, Y = ac.rows(c)
    net = make_net(gnn, oracle_mod, c, dtype)
    net.upload_dataset(X, Y)
    for baseline in ic.BASELINES:
        ig, delta = net.integrated_gradients_range(M, baseline, delta=True)
        assert delta.shape == (c.n,) and delta.dtype == np.float64
        assert same_bits(ig, net.integrated_gradients_range(M, baseline))
        # the same identity from the host: calculateLoss in the same blocks, the cells summed by numpy
        host = gnn.convergence_delta(net, X, Y, ig, baseline)
        lx = block_losses(net, X, Y, c.max_batch)
        lb = block_losses(net, np.full(X.shape, float(np.float32(baseline))), Y, c.max_batch)
        order = c.dims[0] * 2.0 ** -52 * np.abs(ig).sum(axis=1) + 2.0 ** -51 * (np.abs(ig.sum(axis=1)) + np.abs(lx - lb))
        print("%s %d b=%.2f: worst |delta| %.3g, |delta - host| %.3g (the sum's order %.3g)"
              % (name, dtype, baseline, np.abs(delta).max(), np.abs(delta - host).max(), order.max()))
        assert np.all(np.abs(delta - host) <= order)
        if dtype == F32:
            bound = ic.delta_bound(oracle_mod, c, baseline, lx, lb)
            gap = float(np.abs(ic.model_gap(oracle_mod, c, baseline)).max())
            print("   model gap %.3g, worst |delta| / bound %.3g" % (gap, (np.abs(delta) / bound).max()))
            assert np.all(np.abs(delta) <= bound)
        assert np.array_equal(bits(net.integrated_gradients_range(M, baseline, delta=True)[1]), bits(delta))     # the same bits every time


# ---- 4. maps ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", [("relu_zeros", F32), ("blocks", F32), ("blocks_dense", BF16), ("gemm_plan", F32)])
def test_maps_are_the_row_order_sums(gnn, oracle_mod, name, dtype):
    c = ac.BY_NAME[name]
    X, Y = ac.rows(c)
    net = make_net(gnn, oracle_mod, c, dtype)
    net.upload_dataset(X, Y)
    ig, maps, class_rows = net.integrated_gradients_range(M, 0.25, maps=True)
    d_out = c.dims[-1]
    e = expected_rule(Y)
    want = np.zeros((d_out, c.dims[0]))
    for r in range(c.n):                                      # ONE sum per cell, in row order, in fp64
        want[e[r]] += np.abs(ig[r])
    assert maps.shape == want.shape and np.array_equal(bits(maps), bits(want))
    assert class_rows.dtype == np.int64 and np.array_equal(class_rows, np.bincount(e, minlength=d_out))
    assert maps.max() > 0
    # every output on its own, and all four together, carry the same bits
    lib, h = net._lib, net._h
    m2, r2 = np.zeros_like(maps), np.zeros(d_out, dtype=np.int64)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    gnn._capi.check(lib.gnn_mlp_integrated_gradients_set_range(h, 0, 0, c.n, M, 0.25, None, dp(m2), None, None))
    gnn._capi.check(lib.gnn_mlp_integrated_gradients_set_range(h, 0, 0, c.n, M, 0.25, None, None, r2.ctypes.data_as(C.POINTER(C.c_int64)), None))
    assert np.array_equal(bits(m2), bits(maps)) and np.array_equal(r2, class_rows)
    ig4, maps4, rows4, delta4 = net.integrated_gradients_range(M, 0.25, maps=True, delta=True)
    assert same_bits(ig4, ig) and np.array_equal(bits(maps4), bits(maps)) and np.array_equal(rows4, class_rows)
    assert np.array_equal(bits(delta4), bits(net.integrated_gradients_range(M, 0.25, delta=True)[1]))


# ---- 5. ranges ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", [("relu_zeros", F32), ("blocks", F32), ("blocks_dense", BF16), ("per_layer", F32), ("gemm_plan", BF16)])
def test_ranges_and_the_held_out_set(gnn, oracle_mod, name, dtype):
    c = ac.BY_NAME[name]
    X, Y = ac.rows(c)
    Xh, Yh = ac.held_rows(c)
    net, twin = make_net(gnn, oracle_mod, c, dtype), make_net(gnn, oracle_mod, c, dtype)
    net.upload_dataset(X, Y)
    net.upload_held_out(Xh, Yh)
    twin.upload_dataset(Xh, Yh)
    g_before = net.input_gradient_range()
    whole, delta = net.integrated_gradients_range(M, 0.25, delta=True)
    # the held-out rows as a net of the same weights attributes them as ITS training set; the training set's results stay
    held = net.integrated_gradients_range(M, 0.25, held_out=True, maps=True, delta=True)
    want = twin.integrated_gradients_range(M, 0.25, maps=True, delta=True)
    assert same_bits(held[0], want[0]) and np.array_equal(bits(held[1]), bits(want[1])) and np.array_equal(held[2], want[2])
    assert np.array_equal(bits(held[3]), bits(want[3]))
    assert same_bits(held[0], host_route(gnn, net, Xh, Yh, 0, c.n, c.max_batch, M, 0.25))
    if dtype == F32:
        ref = ic.reference(oracle_mod, c, 0.25, False, M, held=True)
        assert np.all(np.abs(held[0] - ref.ig) <= ref.budget)
    # two identical calls in a row: no stale sum, whatever the call between them left
    again, delta2 = net.integrated_gradients_range(M, 0.25, delta=True)
    assert same_bits(again, whole) and np.array_equal(bits(delta2), bits(delta))
    net.integrated_gradients_range(3, 0.0)
    assert same_bits(net.integrated_gradients_range(M, 0.25), whole)
    if c.n > c.max_batch:      # a sub-range that starts on a block boundary: the bits of the matching rows of the whole range
        first = c.max_batch
        part, dpart = net.integrated_gradients_range(M, 0.25, first, c.n - first, delta=True)
        assert same_bits(part, whole[first:]) and np.array_equal(bits(dpart), bits(delta[first:]))
        part = net.integrated_gradients_range(M, 0.25, first, 5)
        assert same_bits(part, whole[first:first + 5])
    # the shared gx buffer: input_gradient_range returns what it returned before
    assert np.array_equal(net.input_gradient_range(), g_before)


# ---- 6. nothing moves -----------------------------------------------------------------------------------------------------------------
def _state(net):
    return net.get_weights(), net.get_momentum(), net.time


def _same_state(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


@pytest.mark.parametrize("name,dtype,env,launches", [("blocks", F32, None, 2), ("blocks_dense", BF16, None, 2), ("blocks", F32, "GNN_MLP_CHAIN", 3)])
def test_nothing_moves(gnn, oracle_mod, monkeypatch, name, dtype, env, launches):
    """Weights, momentum and time after training are bitwise those of the run without the calls: between two train_range calls,
    with a host-batch gradientStep's update pending, and inside a train_sampled run cut in two (the settings of
    tests/test_input_gradient_gpu.py); the calls themselves leave weights, momentum, step count and sampler as they were."""
    import os
    if os.environ.get("GNN_MLP_PATH"):
        pytest.skip("path forced by the environment")
    if env:
        monkeypatch.setenv(env, "0")
    c = ac.BY_NAME[name]
    B, n = 8, 96
    X, Y = ac.make_rows(c.dims, n, c.seed + 200, c.density)

    def run(ask):
        net = make_net(gnn, oracle_mod, c, dtype, max_batch=B)
        assert net.step_launches == launches, net.plan_note
        net.upload_dataset(X, Y)
        net.upload_held_out(X[:20], Y[:20])
        out = []
        net.train_range(0, B, 5, 0.05, 0.9)
        if ask:
            before = _state(net)
            net.integrated_gradients_range(M, 0.0, 0, n)
            net.integrated_gradients_range(1, 0.25, 0, n, delta=True)
            net.integrated_gradients_range(3, 0.25, 0, n, maps=True, delta=True)
            _same_state(before, _state(net))
        net.train_range(5 * B, B, 5, 0.05, 0.9)
        out.append(_state(net))
        net.gradientStep(X[:B], 0.05, 0.9, False, expected=Y[:B])
        if ask:
            net.integrated_gradients_range(M, 0.25, B, 2 * B + 3)
            net.integrated_gradients_range(M, 0.0, held_out=True, delta=True)
        net.gradientStep(X[B:2 * B], 0.05, 0.9, False, expected=Y[B:2 * B])
        out.append(_state(net))
        smp = gnn.Sampler(n, seed=3)
        net.train_sampled(smp, 6, B, 0.05, 0.9)
        if ask:
            net.integrated_gradients_range(2, 0.25, 5, n - 5, maps=True)
            net.integrated_gradients_range(M, 0.0, held_out=True)
            net.integrated_gradients_range(1, 0.0, 0, 2 * B, delta=True)
        net.train_sampled(smp, 6, B, 0.05, 0.9)
        out.append(_state(net))
        out.append(smp.sample(B))
        return out

    with_calls, without = run(True), run(False)
    assert without[0][2] == 10 and without[2][2] == 24
    for x, y in zip(with_calls[:3], without[:3]):
        _same_state(x, y)
    assert np.array_equal(with_calls[3], without[3])


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------
def _refused(gnn, code, fn):
    with pytest.raises(gnn.GnnError) as e:
        fn()
    assert e.value.code == code, (e.value.code, str(e.value))
    return str(e.value)


def test_refusals_leave_the_net_alone(gnn, oracle_mod):
    c = ac.BY_NAME["ident"]
    X, Y = ac.rows(c)
    capi = gnn._capi
    for inner in (ac.SIGMOID, ac.TANH):     # the device holds f(x), not x
        net = gnn.SoftmaxCrossEntropyNeuralNet(c.dims, inner_act=inner, max_batch=c.n)
        net.upload_dataset(X, Y)
        before = _state(net)
        assert "f(x)" in _refused(gnn, capi.ERR_UNSUPPORTED, lambda: net.integrated_gradients_range(M))
        _same_state(before, _state(net))
        assert gnn.integrated_gradients(net, X[:4], Y[:4], 2).shape == (4, c.dims[0])      # the host route serves it
    net, twin = make_net(gnn, oracle_mod, c), make_net(gnn, oracle_mod, c)
    _refused(gnn, capi.ERR_STATE, lambda: net.integrated_gradients_range(M, 0.0, 0, 4))       # no data set uploaded
    _refused(gnn, capi.ERR_STATE, lambda: net.integrated_gradients_range(M, 0.0, 0, 4, held_out=True))
    net.upload_dataset(X, Y)
    twin.upload_dataset(X, Y)
    # every refusal below stands behind a host-batch step whose update is still pending: it is applied, nothing else happens
    for n_ in (net, twin):
        n_.gradientStep(X[:8], 0.05, 0.9, False, expected=Y[:8])
    bad = [dict(steps=0), dict(steps=1025), dict(steps=-1), dict(baseline=-0.25), dict(baseline=float("nan")), dict(baseline=float("inf"))]
    for kw in bad:
        p = dict(steps=M, baseline=0.0)
        p.update(kw)
        _refused(gnn, capi.ERR_BAD_ARG, lambda: net.integrated_gradients_range(p["steps"], p["baseline"], 0, 4))
        _refused(gnn, capi.ERR_BAD_ARG, lambda: net.integrated_gradients_range(p["steps"], p["baseline"], 0, 4, maps=True, delta=True))
        net.gradientStep(X[8:16], 0.05, 0.9, False, expected=Y[8:16])       # (a pending update in front of the next refusal)
        twin.gradientStep(X[8:16], 0.05, 0.9, False, expected=Y[8:16])
    for first, n in ((0, c.n + 1), (-1, 2), (c.n, 1), (0, 0)):      # rows outside the set
        _refused(gnn, capi.ERR_BAD_ARG, lambda: net.integrated_gradients_range(M, 0.0, first, n))
    _refused(gnn, capi.ERR_STATE, lambda: net.integrated_gradients_range(M, 0.0, 0, 4, held_out=True))      # no held-out set
    lib, h = net._lib, net._h
    out = np.empty((4, c.dims[0]))
    dp = out.ctypes.data_as(C.POINTER(C.c_double))
    _refused(gnn, capi.ERR_BAD_ARG, lambda: capi.check(lib.gnn_mlp_integrated_gradients_set_range(h, 0, 0, 4, M, 0.0, None, None, None, None)))
    _refused(gnn, capi.ERR_BAD_ARG, lambda: capi.check(lib.gnn_mlp_integrated_gradients_set_range(h, 2, 0, 4, M, 0.0, dp, None, None, None)))   # a set that is neither
    _same_state(_state(twin), _state(net))
    assert net.time == 1 + len(bad)
    # the limits themselves are served, and the handle is usable
    assert net.integrated_gradients_range(1, 0.0, 0, 4).shape == (4, c.dims[0])
    assert same_bits(net.integrated_gradients_range(M, 0.25), host_route(gnn, net, X, Y, 0, c.n, c.max_batch, M, 0.25))
    # members of a group and replicas are out of scope
    grp = gnn.NetGroup(c.dims, [1, 2], inner_act=c.inner, max_batch=c.n)
    grp.upload_dataset(X, Y)
    _refused(gnn, capi.ERR_STATE, lambda: grp.members[0].integrated_gradients_range(M, 0.0, 0, 4))
    dpn = gnn.DataParallelNeuralNet(c.dims, devices=[0, 0], inner_act=c.inner, max_batch=2 * c.n, reducer=gnn.REDUCE_DIRECT)
    _refused(gnn, capi.ERR_STATE, lambda: dpn.replicas[0].integrated_gradients_range(M, 0.0, 0, 4))


def test_the_largest_step_count_is_served(gnn, oracle_mod):
    """steps = 1024 on four rows, against the host route bit for bit"""
    c = ac.BY_NAME["per_layer"]
    X, Y = ac.rows(c)
    net = make_net(gnn, oracle_mod, c)
    net.upload_dataset(X, Y)
    ig = net.integrated_gradients_range(1024, 0.25, 0, 4)
    assert same_bits(ig, gnn.integrated_gradients(net, X[:4], Y[:4], 1024, 0.25))
