"""Input gradients on the device (gnn_mlp_input_gradient, gnn_mlp_input_gradient_range, gnn_mlp_group_input_gradient_range;
csrc/input_grad_kernel.h) against the fp64 restatement of tests/input_gradient_cases.py on the oracle's weights.

Budgets (set before any run, from the budgets the weight gradients have): f32 |g - g_ref| <= 2e-5 max|g_ref| + 1e-9 over the
call (test_parity_gpu.py); bf16 4e-3 max|g_ref| + 1e-7 against the bf16 restatement (test_bf16_gpu.py), on the fixtures whose
own scatter tests/test_input_gradient_cpu.py holds below half of that.  Everything about blocks, consumers, groups and
"nothing moves" is bitwise."""
import ctypes as C

import numpy as np
import pytest

from tests import input_gradient_cases as igc
from tests import np_oracle as npo

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1


def make_net(gnn, c, dtype=F32, max_batch=None, seed=1):
    mb = max_batch or c.B
    if c.out_kind == igc.SCE:
        return gnn.SoftmaxCrossEntropyNeuralNet(c.dims, inner_act=c.inner, seed=seed, dtype=dtype, max_batch=mb)
    return gnn.GeneralNeuralNet(c.dims, inner_act=c.inner, last_act=c.last, seed=seed, dtype=dtype, max_batch=mb)


def check_budget(g, ref, bf16=False, what=""):
    err, bound = igc.within(g, ref, bf16)
    print("%s worst |g - g_ref| %.3g, budget %.3g (%.3g max|g_ref|)" % (what, err, bound, err / np.abs(ref).max()))
    assert err <= bound, (what, err, bound)


def expected_rule(Y):
    """MT:186-188: the LAST index whose expected value is exactly 1, 0 when there is none."""
    return np.array([int(np.flatnonzero(r == 1.0)[-1]) if (r == 1.0).any() else 0 for r in np.asarray(Y)], dtype=np.int64)


def saliency_of(grad, Y):
    """the fp64 sum of |grad| by expected class, and the rows per class"""
    d = Y.shape[1]
    e = expected_rule(Y)
    sal = np.zeros((d, grad.shape[1]))
    for c in range(d):
        sal[c] = np.abs(grad[e == c]).sum(axis=0)
    return sal, np.bincount(e, minlength=d).astype(np.int64)


def check_saliency(sal, rows, grad, Y):
    want, want_rows = saliency_of(grad, Y)
    assert np.array_equal(rows, want_rows)
    assert np.all(np.abs(sal - want) <= 1e-12 * np.abs(want))


# ---- 1. the product against the restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in igc.CASES])
def test_f32_within_budget(gnn, oracle_mod, name):
    c = igc.BY_NAME[name]
    X, Y = igc.batch(c)
    ref = igc.reference(oracle_mod, c)
    net = make_net(gnn, c)
    if name in ("baseline", "headline"):
        assert net.step_launches == 2, net.plan_note
    if name == "gemm_plan":     # refused by the two-launch plan (more than 16 first-layer K slabs)
        assert net.step_launches != 2 and net.plan_note
    if name == "two_layer":     # per-layer GEMMs
        assert net.step_launches == 0 and net.plan_note
    g = net.input_gradient(X, Y)
    assert g.shape == X.shape and g.dtype == np.float64
    check_budget(g, ref, what=name)
    # a single row gets a 1-D result; it is row 0 of the batch call within the budget
    g0 = net.input_gradient(X[0], Y[0])
    assert g0.shape == (c.dims[0],)
    assert np.abs(g0 - g[0]).max() <= igc.F32_RTOL * np.abs(ref).max() + igc.F32_ATOL


@pytest.mark.parametrize("name", [c.name for c in igc.BF16_CASES])
def test_bf16_within_budget(gnn, oracle_mod, name):
    c = igc.BY_NAME[name]
    X, Y = igc.batch(c)
    net = make_net(gnn, c, dtype=BF16)
    check_budget(net.input_gradient(X, Y), igc.reference(oracle_mod, c, bf16=True), bf16=True, what=name + " bf16")


def test_exact_zero_inputs_take_the_left_branch(gnn, oracle_mod):
    """MT:235 on the device: at an exact-zero input the leaky factor is 0.01 -- the entries there are a hundredth of what the
    wrong rule (`a < 0`) would leave, which tests/test_input_gradient_cpu.py holds to be ~0.8 max|g| away."""
    c = igc.BY_NAME["zeros"]
    X, Y = igc.batch(c)
    g = make_net(gnn, c).input_gradient(X, Y)
    wrong = igc.input_gradient(igc.weights(oracle_mod, c), X, Y, c.inner, c.out_kind, c.last, input_prime=igc.wrong_rule_prime)
    assert np.abs(g - wrong).max() > 0.1 * np.abs(wrong).max()


# ---- 2. host batch, range, blocks, consumers ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", [("ragged", F32), ("baseline", F32), ("general", F32), ("gemm_plan", F32), ("two_layer", F32),
                                        ("zeros", BF16)])
def test_host_batch_and_range_give_the_same_bits(gnn, name, dtype):
    c = igc.BY_NAME[name]
    X, Y = igc.batch(c)
    net = make_net(gnn, c, dtype=dtype)
    net.upload_dataset(X, Y)
    host = net.input_gradient(X, Y)
    rng = net.input_gradient_range(0, c.B)
    assert rng.shape == host.shape
    assert np.array_equal(host, rng)
    assert np.array_equal(net.input_gradient_range(), rng)   # n=None: the whole data set


@pytest.mark.parametrize("name,dtype,mb", [("ragged", F32, 8), ("zeros", BF16, 7), ("baseline", F32, 13), ("gemm_plan", F32, 6)])
def test_a_range_is_its_blocks(gnn, name, dtype, mb):
    """n = 2 max_batch + 3 rows: two full blocks and a ragged one."""
    c = igc.BY_NAME[name]
    n = 2 * mb + 3
    X, Y = igc.make_rows(c.dims, n, c.seed + 100, c.density)
    net = make_net(gnn, c, dtype=dtype, max_batch=mb)
    net.upload_dataset(X, Y)
    g, sal, rows = net.input_gradient_range(0, n, grad=True, saliency=True)
    assert g.shape == (n, c.dims[0]) and sal.shape == (c.dims[-1], c.dims[0]) and rows.dtype == np.int64
    blocks = np.concatenate([net.input_gradient_range(off, min(mb, n - off)) for off in range(0, n, mb)])
    assert np.array_equal(g, blocks)
    assert np.abs(g).max() > 0
    check_saliency(sal, rows, g, Y)     # the accumulation, not the product: against the fp64 sum of the returned rows
    assert rows.sum() == n
    # the same call again: the same bits; the saliency-only form: the same map
    g2, sal2, rows2 = net.input_gradient_range(0, n, grad=True, saliency=True)
    assert np.array_equal(g, g2) and np.array_equal(sal, sal2) and np.array_equal(rows, rows2)
    sal3, rows3 = net.input_gradient_range(0, n, grad=False, saliency=True)
    assert np.array_equal(sal, sal3) and np.array_equal(rows, rows3)
    # a range that starts inside the data set
    assert np.array_equal(net.input_gradient_range(3, n - 5), g[3:n - 2])


def test_lone_call_errors(gnn):
    c = igc.BY_NAME["ragged"]
    X, Y = igc.batch(c)
    net = make_net(gnn, c)
    with pytest.raises(gnn.GnnError) as e:
        gnn._capi.check(net._lib.gnn_mlp_input_gradient_range(net._h, 0, 4, np.empty((4, 20)).ctypes.data_as(C.POINTER(C.c_double)), None, None))
    assert e.value.code == gnn._capi.ERR_STATE      # no data set
    net.upload_dataset(X, Y)
    for first, n in ((0, c.B + 1), (-1, 2), (c.B, 1), (0, 0)):
        with pytest.raises(gnn.GnnError) as e:
            gnn._capi.check(net._lib.gnn_mlp_input_gradient_range(net._h, first, n, np.empty((c.B + 1, 20)).ctypes.data_as(C.POINTER(C.c_double)), None, None))
        assert e.value.code == gnn._capi.ERR_BAD_ARG
    with pytest.raises(gnn.GnnError) as e:
        gnn._capi.check(net._lib.gnn_mlp_input_gradient_range(net._h, 0, c.B, None, None, None))
    assert e.value.code == gnn._capi.ERR_BAD_ARG    # every output null
    with pytest.raises(gnn.GnnError) as e:
        net.input_gradient(np.zeros((c.B + 1, 20)), np.zeros((c.B + 1, 7)))
    assert e.value.code == gnn._capi.ERR_BAD_ARG    # B above max_batch


# ---- 3. plans -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype,env,launches", [
    ("baseline", F32, "GNN_MLP_CHAIN", 3),       # three launches per step
    ("zeros", F32, "GNN_MLP_ROWBLOCK", 2),       # two launches, middle4_kernel as the row-block kernel
    ("baseline", BF16, "GNN_MLP_CHAIN", 0),      # bf16 off the two-launch path: per-layer bf16 GEMMs with the tail kernel
    ("gemm_plan", F32, None, 3),                 # the two-launch plan refuses the net
    ("two_layer", F32, None, 0),                 # per-layer f32 GEMMs
])
def test_plans(gnn, oracle_mod, monkeypatch, name, dtype, env, launches):
    import os
    if os.environ.get("GNN_MLP_PATH"):
        pytest.skip("path forced by the environment")
    if env:
        monkeypatch.setenv(env, "0")
    c = igc.BY_NAME[name]
    X, Y = igc.batch(c)
    net = make_net(gnn, c, dtype=dtype)
    assert net.step_launches == launches, net.plan_note
    if env == "GNN_MLP_ROWBLOCK":
        assert net.rowblock_state == 0
    g = net.input_gradient(X, Y)
    check_budget(g, igc.reference(oracle_mod, c, bf16=dtype == BF16), bf16=dtype == BF16, what="%s %s=0" % (name, env))
    net.upload_dataset(X, Y)
    assert np.array_equal(net.input_gradient_range(0, c.B), g)


def test_hybrid_plan(gnn, oracle_mod):
    """middle weights beyond one workgroup's LDS: the one-launch first layer / gradient around per-layer GEMMs"""
    import os
    if os.environ.get("GNN_MLP_PATH") or os.environ.get("GNN_MLP_HYBRID"):
        pytest.skip("path forced by the environment")
    dims, B = [200, 512, 272, 10], 27
    X, Y = igc.make_rows(dims, B, 77, 0.19)
    net = gnn.SoftmaxCrossEntropyNeuralNet(dims, max_batch=B)
    assert "do not fit" in net.plan_note
    ref = igc.input_gradient(npo.split(oracle_mod.OracleNet(dims).get_weights(), dims), X, Y, igc.LEAKY)
    check_budget(net.input_gradient(X, Y), ref, what="hybrid")


def test_data_parallel_replica(gnn, oracle_mod):
    """a borrowed handle of the other kind: a replica of a data-parallel net (two replicas sharing the device)"""
    c = igc.BY_NAME["zeros"]
    X, Y = igc.batch(c)
    dp = gnn.DataParallelNeuralNet(c.dims, devices=[0, 0], inner_act=c.inner, max_batch=2 * c.B, reducer=gnn.REDUCE_DIRECT)
    g = dp.replicas[1].input_gradient(X[:8], Y[:8])
    ref = igc.reference(oracle_mod, c)
    assert np.abs(g - ref[:8]).max() <= igc.F32_RTOL * np.abs(ref).max() + igc.F32_ATOL
    assert np.array_equal(dp.replicas[0].input_gradient(X[:8], Y[:8]), g)


# ---- 4. nothing moves -----------------------------------------------------------------------------------------------------------
def _state(net):
    return net.get_weights(), net.get_momentum(), net.time


def _same_state(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def _train_sampled(gnn, net, smp, iters, B):
    gnn._capi.check(net._lib.gnn_mlp_train_sampled(net._h, smp._h, iters, B, 0.05, 0.9, 0))


@pytest.mark.parametrize("name,dtype", [("zeros", F32), ("zeros", BF16), ("gemm_plan", F32)])
def test_nothing_moves(gnn, name, dtype):
    """Weights, momentum and time after training are bitwise those of the run without the calls: between two train_range calls,
    with a host-batch gradientStep's update pending, and inside a train_sampled run cut in two."""
    c = igc.BY_NAME[name]
    B, n = 8, 96
    X, Y = igc.make_rows(c.dims, n, c.seed + 200, c.density)

    def run(ask):
        net = make_net(gnn, c, dtype=dtype, max_batch=B)
        net.upload_dataset(X, Y)
        out = []
        # between two train_range calls
        net.train_range(0, B, 5, 0.05, 0.9)
        if ask:
            net.input_gradient_range(0, n, grad=True, saliency=True)
        net.train_range(5 * B, B, 5, 0.05, 0.9)
        out.append(_state(net))
        # a host-batch step whose update is deferred into the next call
        net.gradientStep(X[:B], 0.05, 0.9, False, expected=Y[:B])
        if ask:
            net.input_gradient_range(B, 2 * B + 3)
            net.input_gradient(X[3:3 + B], Y[3:3 + B])
        net.gradientStep(X[B:2 * B], 0.05, 0.9, False, expected=Y[B:2 * B])
        out.append(_state(net))
        # a sampled run cut in two
        smp = gnn.Sampler(n, seed=3)
        _train_sampled(gnn, net, smp, 6, B)
        if ask:
            net.input_gradient_range(0, n, grad=False, saliency=True)
        _train_sampled(gnn, net, smp, 6, B)
        out.append(_state(net))
        return out

    with_calls, without = run(True), run(False)
    assert without[0][2] == 10 and without[2][2] == 24
    for a, b in zip(with_calls, without):
        _same_state(a, b)


# ---- 5. groups ------------------------------------------------------------------------------------------------------------------
def _group(gnn, c, K, mb, n, dtype=F32):
    X, Y = igc.make_rows(c.dims, n, c.seed + 300, c.density)
    g = gnn.NetGroup(c.dims, list(range(1, K + 1)), out_kind=gnn.OUT_SOFTMAX_CE, inner_act=c.inner, dtype=dtype, max_batch=mb)
    g.upload_dataset(X, Y)
    return g, X, Y


@pytest.mark.parametrize("name,K,mb", [("baseline", 3, 16), ("gemm_plan", 2, 6), ("baseline", 1, 16)])
def test_group_members_and_ensemble(gnn, oracle_mod, name, K, mb):
    c = igc.BY_NAME[name]
    n = 2 * mb + 3
    g, X, Y = _group(gnn, c, K, mb, n)
    member, ens, msal, esal, rows = g.input_gradient_range(0, n, members=True, saliency=True)
    assert member.shape == (K, n, c.dims[0]) and ens.shape == (n, c.dims[0])
    assert msal.shape == (K, c.dims[-1], c.dims[0]) and esal.shape == (c.dims[-1], c.dims[0])
    for k in range(K):   # member k: bitwise the lone call on the borrowed handle
        lg, lsal, lrows = g.members[k].input_gradient_range(0, n, grad=True, saliency=True)
        assert np.array_equal(member[k], lg)
        assert np.array_equal(msal[k], lsal)
        assert np.array_equal(rows, lrows)
        check_saliency(msal[k], rows, member[k], Y)
    # ... and member K - 1 is the restatement's on Random(K)'s weights
    ref = igc.input_gradient(igc.weights(oracle_mod, c, seed=K), X, Y, c.inner, c.out_kind, c.last)
    check_budget(member[K - 1], ref, what="%s member %d" % (name, K - 1))
    # the ensemble: s = g_0; s += g_k in member order; s / (float)K, in f32
    m32 = member.astype(np.float32)
    assert np.array_equal(m32.astype(np.float64), member)
    s = m32[0].copy()
    for k in range(1, K):
        s = s + m32[k]
    want = s / np.float32(K)
    assert want.dtype == np.float32
    assert np.array_equal(ens, want.astype(np.float64))
    check_saliency(esal, rows, ens, Y)
    # the Python forms that ask for less
    assert np.array_equal(g.input_gradient_range(0, n), ens)
    e2, esal2, rows2 = g.input_gradient_range(0, n, saliency=True)
    assert np.array_equal(e2, ens) and np.array_equal(esal2, esal) and np.array_equal(rows2, rows)


def test_group_outputs_one_at_a_time(gnn):
    """every output null is an error; each output alone is what the full call returns"""
    c = igc.BY_NAME["ragged"]
    K, mb = 2, 8
    n = 2 * mb + 3
    g, X, Y = _group(gnn, c, K, mb, n)
    d0, d = c.dims[0], c.dims[-1]
    full = g.input_gradient_range(0, n, members=True, saliency=True)
    shapes = [((K, n, d0), np.float64), ((n, d0), np.float64), ((K, d, d0), np.float64), ((d, d0), np.float64), ((d,), np.int64)]
    fn = g._lib.gnn_mlp_group_input_gradient_range

    def ptr(a):
        return a.ctypes.data_as(C.POINTER(C.c_int64 if a.dtype == np.int64 else C.c_double))

    with pytest.raises(gnn.GnnError) as e:
        gnn._capi.check(fn(g._h, 0, n, None, None, None, None, None))
    assert e.value.code == gnn._capi.ERR_BAD_ARG
    for i, (shape, dt) in enumerate(shapes):
        out = np.full(shape, -7, dtype=dt)
        args = [None] * 5
        args[i] = ptr(out)
        gnn._capi.check(fn(g._h, 0, n, *args))
        assert np.array_equal(out, full[i]), i
    with pytest.raises(gnn.GnnError) as e:
        gnn._capi.check(fn(g._h, 1, n, None, ptr(np.empty((n, d0))), None, None, None))
    assert e.value.code == gnn._capi.ERR_BAD_ARG    # rows outside the data set


# ---- 6. fgsm ----------------------------------------------------------------------------------------------------------------------
def test_fgsm_raises_the_loss(gnn):
    """A direction check, no threshold beyond `>`: on a briefly trained net the mean loss on the perturbed rows is above the mean
    loss on the rows.  (The same rows, steps and seed on the CPU with the restatement: test_fgsm_direction_on_the_cpu in tests/test_input_gradient_cpu.py.)"""
    c = igc.BY_NAME["zeros"]
    n, B, steps, step, momentum, eps = igc.FGSM
    X, Y = igc.make_rows(c.dims, n, c.seed + 400, c.density)
    net = make_net(gnn, c, max_batch=n)
    net.upload_dataset(X, Y)
    net.train_range(0, B, steps, step, momentum)
    adv = gnn.fgsm(net, X, Y, eps)
    assert adv.shape == X.shape and adv.min() >= 0.0 and adv.max() <= 1.0
    assert np.abs(adv - X).max() <= eps + 1e-15
    before, after = net.calculateLoss(X, Y).mean(), net.calculateLoss(adv, Y).mean()
    print("mean loss %.4g -> %.4g" % (before, after))
    assert after > before
