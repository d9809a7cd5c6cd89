"""The fast-gradient-sign calls on the device (gnn_mlp_fgsm_set_range, gnn_mlp_evaluate_fgsm_set_range,
gnn_mlp_train_sampled_fgsm; csrc/adversarial.hip, csrc/input_grad_kernel.h: fgsm_kernel) on the fixtures of
tests/adversarial_cases.py.

Exact twins (bit for bit): the perturbed rows against the formula in numpy float32 on the gradient the device itself returns;
robust hits against argmax on those rows fed back as host batches; adversarial training against a host-driven loop of
input_gradient, the float32 perturbation and gradientStep; "nothing moves" around the two range calls.
Against the fp64 model: every decided element (tests/adversarial_cases.py; tests/test_adversarial_cpu.py holds the undecided
ones below 5 %) is the model's value rounded to float32; the robust loss within the budget test_group_eval_gpu.py gives a
loss sum against summed per-row losses (1e-4 |l| + 1e-5 per row); the 40-iteration oracle run within W_ATOL = 2e-6 per step."""
import ctypes as C

import numpy as np
import pytest

from tests import adversarial_cases as ac

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1
EVERY = [(c.name, dt) for c in ac.CASES for dt in (F32, BF16)]
WITH_ORACLE = [(c.name, F32) for c in ac.CASES] + [(c.name, BF16) for c in ac.BF16_CASES]


def make_net(gnn, oracle_mod, c, dtype=F32, max_batch=None):
    net = gnn.SoftmaxCrossEntropyNeuralNet(c.dims, inner_act=c.inner, seed=1, dtype=dtype, max_batch=max_batch or c.max_batch)
    net.set_weights(ac.flat_weights(oracle_mod, c))
    return net


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def f32_twin(X, g, eps, clip=ac.CLIP):
    return ac.perturb(X, g, eps, clip, dtype=np.float32)


def expected_rule(Y):
    """MT:186-188: the LAST index whose expected value is exactly 1, 0 when there is none."""
    return np.array([int(np.flatnonzero(r == 1.0)[-1]) if (r == 1.0).any() else 0 for r in np.asarray(Y)], dtype=np.int64)


# ---- 1. rows, exact twin ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", EVERY)
def test_rows_are_the_float32_formula_on_the_device_gradient(gnn, oracle_mod, name, dtype):
    c = ac.BY_NAME[name]
    X, Y = ac.rows(c)
    net = make_net(gnn, oracle_mod, c, dtype)
    net.upload_dataset(X, Y)
    g = net.input_gradient_range(0, c.n)
    assert np.abs(g).max() > 0
    for eps in ac.EPS:
        adv = net.fgsm_range(eps, 0, c.n)
        assert adv.shape == X.shape and adv.dtype == np.float64
        assert same_bits(adv, f32_twin(X, g, eps)), (name, eps, int((adv != f32_twin(X, g, eps)).sum()))
    assert same_bits(net.fgsm_range(0.0), X)                       # eps = 0: the rows, bit for bit
    assert np.array_equal(net.fgsm_range(0.1), adv)                # n=None: the whole set; the same bits every time
    if c.n > 8:                                                    # a range that starts inside the set
        assert np.array_equal(net.fgsm_range(0.1, 3, c.n - 5), adv[3:c.n - 2])
    if c.inner == ac.RELU:                                         # g == 0 exactly: the pixel stays 0
        assert np.all(adv[X == 0.0] == 0.0) and (X == 0.0).mean() > 0.4
    clip = (0.125, 0.875)                                          # a clip that acts on a fifth of the elements
    assert same_bits(net.fgsm_range(0.1, clip=clip), f32_twin(X, g, 0.1, clip))
    # the gradient call behind the perturbation returns what it returned before
    assert np.array_equal(net.input_gradient_range(0, c.n), g)


@pytest.mark.parametrize("name,dtype", [("relu_zeros", F32), ("blocks", F32), ("blocks_dense", BF16), ("per_layer", F32), ("gemm_plan", BF16)])
def test_rows_of_the_held_out_set(gnn, oracle_mod, name, dtype):
    """the held-out rows perturbed as a net of the same weights perturbs them as ITS training set; the training set's results
    are not disturbed"""
    c = ac.BY_NAME[name]
    X, Y = ac.rows(c)
    Xh, Yh = ac.held_rows(c)
    net, twin = make_net(gnn, oracle_mod, c, dtype), make_net(gnn, oracle_mod, c, dtype)
    net.upload_dataset(X, Y)
    net.upload_held_out(Xh, Yh)
    twin.upload_dataset(Xh, Yh)
    gh = twin.input_gradient_range(0, c.n)
    before = net.fgsm_range(0.1)
    adv = net.fgsm_range(0.1, held_out=True)
    assert same_bits(adv, f32_twin(Xh, gh, 0.1))
    assert np.array_equal(adv, twin.fgsm_range(0.1))
    assert net.evaluate_fgsm_range(0.1, held_out=True) == twin.evaluate_fgsm_range(0.1)
    assert np.array_equal(net.fgsm_range(0.1), before)
    assert same_bits(before, f32_twin(X, net.input_gradient_range(0, c.n), 0.1))


# ---- 2. rows against the fp64 model -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", WITH_ORACLE)
def test_decided_elements_are_the_models(gnn, oracle_mod, name, dtype):
    c = ac.BY_NAME[name]
    bf = dtype == BF16
    X, Y = ac.rows(c)
    g = ac.reference_gradient(oracle_mod, c, bf)
    dec = ac.decided(g, X, c.inner, bf)
    net = make_net(gnn, oracle_mod, c, dtype)
    net.upload_dataset(X, Y)
    for eps in ac.EPS:
        adv = net.fgsm_range(eps, 0, c.n)
        want = ac.perturb(X, g, eps).astype(np.float32)
        off = adv.astype(np.float32) != want
        print("%s %s eps %g: %d of %d elements undecided, %d of them off the model; %d decided elements off"
              % (name, "bf16" if bf else "f32", eps, (~dec).sum(), dec.size, (off & ~dec).sum(), (off & dec).sum()))
        assert not (off & dec).any()
    assert (~dec).mean() <= ac.UNDECIDED_CAP


# ---- 3. evaluation ------------------------------------------------------------------------------------------------------------------
def _host_evaluation(net, adv, Y, mb):
    """hits and the fp64 loss sum of the rows fed back as host batches, block by block"""
    hits, losses = 0, []
    e = expected_rule(Y)
    for off in range(0, len(adv), mb):
        rows = slice(off, min(off + mb, len(adv)))
        hits += int((net.argmax(adv[rows]) == e[rows]).sum())
        losses.append(np.atleast_1d(net.calculateLoss(adv[rows], Y[rows])))
    return hits, np.concatenate(losses)


@pytest.mark.parametrize("name,dtype", WITH_ORACLE)
def test_robust_hits_and_loss(gnn, oracle_mod, name, dtype):
    c = ac.BY_NAME[name]
    X, Y = ac.rows(c)
    net = make_net(gnn, oracle_mod, c, dtype)
    net.upload_dataset(X, Y)
    for eps in ac.EPS:
        hits, loss = net.evaluate_fgsm_range(eps, 0, c.n)
        assert (hits, loss) == net.evaluate_fgsm_range(eps)            # the same bits every time
        adv = net.fgsm_range(eps, 0, c.n)
        want_hits, rows_loss = _host_evaluation(net, adv, Y, c.max_batch)
        bound = (1e-4 * np.abs(rows_loss) + 1e-5).sum()
        print("%s %d eps %g: hits %d of %d, loss sum %.9g against %.9g (off by %.3g, budget %.3g)"
              % (name, dtype, eps, hits, c.n, loss, rows_loss.sum(), abs(loss - rows_loss.sum()), bound))
        assert hits == want_hits
        assert abs(loss - rows_loss.sum()) <= bound
        if eps == 0.0:      # the rows themselves: the evaluation pass's loss within the same budget
            assert abs(loss - net.evaluate_range(0, c.n)[1]) <= bound
    assert net.evaluate_fgsm_range(0.1)[1] > net.evaluate_fgsm_range(0.0)[1]     # the perturbation raises the loss
    # ... and on a briefly trained net, where the hits are neither none nor all, the same two comparisons
    B = min(c.n, c.max_batch)
    net.train_range(0, B, 30, 0.05, 0.9)
    clean = net.evaluate_range(0, c.n)[0]
    for eps in (0.02, 0.1):
        hits, loss = net.evaluate_fgsm_range(eps, 0, c.n)
        want_hits, rows_loss = _host_evaluation(net, net.fgsm_range(eps, 0, c.n), Y, c.max_batch)
        print("%s %d trained, eps %g: hits %d of %d (clean %d), loss sum %.9g against %.9g" % (name, dtype, eps, hits, c.n, clean, loss, rows_loss.sum()))
        assert hits == want_hits
        assert abs(loss - rows_loss.sum()) <= (1e-4 * np.abs(rows_loss) + 1e-5).sum()


def _state(net):
    return net.get_weights(), net.get_momentum(), net.time


def _same_state(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


@pytest.mark.parametrize("name,dtype,env,launches", [("blocks", F32, None, 2), ("blocks_dense", BF16, None, 2), ("blocks", F32, "GNN_MLP_CHAIN", 3)])
def test_nothing_moves(gnn, oracle_mod, monkeypatch, name, dtype, env, launches):
    """Weights, momentum and time after training are bitwise those of the run without the calls: between two train_range calls,
    with a host-batch gradientStep's update pending, and inside a train_sampled run cut in two (the settings of
    tests/test_input_gradient_gpu.py)."""
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
            net.evaluate_fgsm_range(0.1, 0, n)
            net.fgsm_range(0.1, 0, n)
        net.train_range(5 * B, B, 5, 0.05, 0.9)
        out.append(_state(net))
        net.gradientStep(X[:B], 0.05, 0.9, False, expected=Y[:B])
        if ask:
            net.fgsm_range(0.1, B, 2 * B + 3)
            net.evaluate_fgsm_range(0.1, held_out=True)
        net.gradientStep(X[B:2 * B], 0.05, 0.9, False, expected=Y[B:2 * B])
        out.append(_state(net))
        smp = gnn.Sampler(n, seed=3)
        net.train_sampled(smp, 6, B, 0.05, 0.9)
        if ask:
            net.evaluate_fgsm_range(0.1, 5, n - 5)
            net.fgsm_range(0.1, held_out=True)
        net.train_sampled(smp, 6, B, 0.05, 0.9)
        out.append(_state(net))
        return out

    with_calls, without = run(True), run(False)
    assert without[0][2] == 10 and without[2][2] == 24
    for a, b in zip(with_calls, without):
        _same_state(a, b)


# ---- 4. training, exact twin ------------------------------------------------------------------------------------------------------
def _train_net(gnn, t, dtype):
    return gnn.SoftmaxCrossEntropyNeuralNet(t.dims, inner_act=t.inner, seed=t.seed, dtype=dtype, max_batch=t.batch)


# (the second clip, with lo > 0, on the batch-8 fixtures: a padding cell that went through the formula would become lo)
TWINS = [(t.name, dt, clip) for t in ac.TWIN_RUNS for dt in (F32, BF16) for clip in (ac.CLIP, (0.125, 0.875)) if clip == ac.CLIP or t.batch == 8]


@pytest.mark.parametrize("run,dtype,clip", TWINS)
def test_training_is_the_host_driven_loop(gnn, run, dtype, clip):
    """40 iterations of gnn_mlp_train_sampled_fgsm against: an identical Sampler, and per iteration input_gradient on the drawn
    rows, the float32 perturbation, gradientStep -- weights, momentum, time and the sampler's state bit for bit."""
    t = [r for r in ac.TWIN_RUNS if r.name == run][0]
    X, Y = ac.train_rows(t)
    step, momentum = ac.TRAIN_HYPER
    net, twin = _train_net(gnn, t, dtype), _train_net(gnn, t, dtype)
    if dtype == F32:
        assert net.step_launches == (2 if run.startswith("two_launch") else 0), net.plan_note
    net.upload_dataset(X, Y)
    smp, smp2 = gnn.Sampler(t.n_rows, seed=ac.SAMPLER_SEED), gnn.Sampler(t.n_rows, seed=ac.SAMPLER_SEED)
    net.train_sampled_fgsm(smp, ac.TRAIN_ITERATIONS, t.batch, step, momentum, ac.TRAIN_EPS, clip)
    drawn = 0
    for _ in range(ac.TRAIN_ITERATIONS):
        idx = smp2.sample(t.batch)
        drawn += len(idx)
        g = twin.input_gradient(X[idx], Y[idx])
        adv = f32_twin(X[idx], g, ac.TRAIN_EPS, clip).astype(np.float64)
        twin.gradientStep(adv, step, momentum, False, expected=Y[idx])
    assert drawn > t.n_rows or t.batch * ac.TRAIN_ITERATIONS <= t.n_rows
    _same_state(_state(net), _state(twin))
    assert net.time == ac.TRAIN_ITERATIONS
    assert np.abs(net.get_weights() - _train_net(gnn, t, dtype).get_weights()).max() > 1e-3    # (it trained)
    for _ in range(3):      # the handle's sampler stands where the twin's stands
        assert np.array_equal(smp.sample(t.batch), smp2.sample(t.batch))


# ---- 5. training against the fp64 model --------------------------------------------------------------------------------------------
def test_training_follows_the_oracle(gnn, oracle_mod):
    """the run tests/test_adversarial_cpu.py::test_the_oracle_run_meets_no_undecided_element holds free of undecided elements"""
    t = ac.ORACLE_RUN
    X, Y = ac.train_rows(t)
    step, momentum = ac.TRAIN_HYPER
    w0 = ac.reference_net(oracle_mod, t.dims, t.inner, t.seed).get_weights()
    w, v, _ = ac.train_model(w0, t, X, Y, ac.draws(gnn, t))
    net = _train_net(gnn, t, F32)
    assert np.abs(net.get_weights() - w0).max() <= 1e-7
    net.upload_dataset(X, Y)
    smp = gnn.Sampler(t.n_rows, seed=ac.SAMPLER_SEED)
    net.train_sampled_fgsm(smp, ac.TRAIN_ITERATIONS, t.batch, step, momentum, ac.TRAIN_EPS)
    bud = ac.W_ATOL * ac.TRAIN_ITERATIONS
    dw, dv = np.abs(net.get_weights() - w).max(), np.abs(net.get_momentum() - v).max()
    print("oracle run: dw %.3g dv %.3g of the budget %.3g" % (dw / bud, dv / bud, bud))
    assert dw <= bud and dv <= bud


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
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
        smp = gnn.Sampler(c.n, seed=1)
        before = _state(net)
        for fn in (lambda: net.fgsm_range(0.1), lambda: net.evaluate_fgsm_range(0.1),
                   lambda: net.train_sampled_fgsm(smp, 3, 8, 0.05, 0.9, 0.1)):
            assert "f(x)" in _refused(gnn, capi.ERR_UNSUPPORTED, fn)
        _same_state(before, _state(net))
        assert np.array_equal(smp.sample(8), gnn.Sampler(c.n, seed=1).sample(8))     # (no draw was taken)
    net = make_net(gnn, oracle_mod, c)
    smp = gnn.Sampler(c.n, seed=1)
    before = _state(net)
    for fn in (lambda: net.fgsm_range(0.1, 0, 4), lambda: net.evaluate_fgsm_range(0.1, 0, 4),
               lambda: net.train_sampled_fgsm(smp, 3, 8, 0.05, 0.9, 0.1),
               lambda: net.fgsm_range(0.1, 0, 4, held_out=True), lambda: net.evaluate_fgsm_range(0.1, 0, 4, held_out=True)):
        _refused(gnn, capi.ERR_STATE, fn)       # no data set uploaded
    net.upload_dataset(X, Y)
    bad = [dict(eps=-0.1), dict(eps=float("inf")), dict(eps=float("nan")), dict(clip=(-0.1, 1.0)), dict(clip=(0.5, 0.25)),
           dict(clip=(float("nan"), 1.0)), dict(clip=(0.0, float("nan")))]
    for kw in bad:
        a = dict(eps=0.1, clip=(0.0, 1.0))
        a.update(kw)
        _refused(gnn, capi.ERR_BAD_ARG, lambda: net.fgsm_range(a["eps"], 0, 4, clip=a["clip"]))
        _refused(gnn, capi.ERR_BAD_ARG, lambda: net.evaluate_fgsm_range(a["eps"], 0, 4, clip=a["clip"]))
        _refused(gnn, capi.ERR_BAD_ARG, lambda: net.train_sampled_fgsm(smp, 3, 8, 0.05, 0.9, a["eps"], clip=a["clip"]))
    for first, n in ((0, c.n + 1), (-1, 2), (c.n, 1), (0, 0)):      # rows outside the set
        _refused(gnn, capi.ERR_BAD_ARG, lambda: net.fgsm_range(0.1, first, n))
        _refused(gnn, capi.ERR_BAD_ARG, lambda: net.evaluate_fgsm_range(0.1, first, n))
    _refused(gnn, capi.ERR_STATE, lambda: net.fgsm_range(0.1, 0, 4, held_out=True))      # no held-out set
    out = np.empty((4, c.dims[0]))
    _refused(gnn, capi.ERR_BAD_ARG, lambda: capi.check(net._lib.gnn_mlp_fgsm_set_range(
        net._h, 2, 0, 4, 0.1, 0.0, 1.0, out.ctypes.data_as(C.POINTER(C.c_double)))))    # a set that is neither
    _refused(gnn, capi.ERR_BAD_ARG, lambda: capi.check(net._lib.gnn_mlp_fgsm_set_range(net._h, 0, 0, 4, 0.1, 0.0, 1.0, None)))
    _refused(gnn, capi.ERR_BAD_ARG, lambda: capi.check(net._lib.gnn_mlp_evaluate_fgsm_set_range(net._h, 0, 0, 4, 0.1, 0.0, 1.0, None, None)))
    # what gnn_mlp_train_sampled refuses: a batch that is the whole set, no iterations, a sampler of another size
    _refused(gnn, capi.ERR_BAD_ARG, lambda: net.train_sampled_fgsm(smp, 3, c.n, 0.05, 0.9, 0.1))
    _refused(gnn, capi.ERR_BAD_ARG, lambda: net.train_sampled_fgsm(smp, 0, 8, 0.05, 0.9, 0.1))
    _refused(gnn, capi.ERR_BAD_ARG, lambda: net.train_sampled_fgsm(gnn.Sampler(c.n + 1, seed=1), 3, 8, 0.05, 0.9, 0.1))
    _same_state(before, _state(net))
    assert np.array_equal(smp.sample(8), gnn.Sampler(c.n, seed=1).sample(8))
    # members of a group are out of scope
    grp = gnn.NetGroup(c.dims, [1, 2], inner_act=c.inner, max_batch=c.n)
    grp.upload_dataset(X, Y)
    _refused(gnn, capi.ERR_STATE, lambda: grp.members[0].fgsm_range(0.1, 0, 4))
