"""The projected-gradient calls on the device (gnn_mlp_pgd_set_range, gnn_mlp_evaluate_pgd_set_range, gnn_mlp_train_sampled_pgd;
csrc/adversarial.hip, csrc/input_grad_kernel.h: pgd_kernel, pgd_start_kernel) on the fixtures of tests/pgd_cases.py.

Exact twins (bit for bit): the start against the definition in numpy uint32 / float32; one step of size eps against fgsm_range;
the attacked rows against gnn_amd.pgd, the host route over the same blocks; the curve against the calls with fewer steps;
adversarial training against a host-driven loop of Sampler.sample, gnn_amd.pgd and gradientStep; "nothing moves" around the range
calls.  Against the fp64 model, teacher-forced on the device's own iterates: every decided element of every step is the model's
value rounded to float32 (tests/test_pgd_cpu.py holds the undecided ones below 5 % per step on the fixtures used here); the robust
loss within the budget test_adversarial_gpu.py gives a loss sum (1e-4 |l| + 1e-5 per row); the oracle run within W_ATOL = 2e-6
per iteration."""
import numpy as np
import pytest

from tests import adversarial_cases as ac
from tests import pgd_cases as pc

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1
TWINS = [(c.name, F32) for c in ac.CASES] + [(c.name, BF16) for c in ac.BF16_CASES]
MODEL = [(name, BF16 if bf else F32) for name, bf in pc.MODEL_CASES]
SEEDS = (None, pc.START_SEED)


def make_net(gnn, oracle_mod, c, dtype=F32, max_batch=None):
    net = gnn.SoftmaxCrossEntropyNeuralNet(c.dims, inner_act=c.inner, seed=1, dtype=dtype, max_batch=max_batch or c.max_batch)
    net.set_weights(ac.flat_weights(oracle_mod, c))
    return net


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def expected_rule(Y):
    """MT:186-188: the LAST index whose expected value is exactly 1, 0 when there is none."""
    return np.array([int(np.flatnonzero(r == 1.0)[-1]) if (r == 1.0).any() else 0 for r in np.asarray(Y)], dtype=np.int64)


def host_route(gnn, net, X, Y, first, n, max_batch, steps=pc.T, clip=pc.CLIP, seed=None, eps=pc.EPS, alpha=pc.ALPHA):
    """gnn_amd.pgd over the blocks of max_batch rows the range call takes"""
    out = []
    for off in range(first, first + n, max_batch):
        rows = slice(off, min(off + max_batch, first + n))
        out.append(gnn.pgd(net, X[rows], Y[rows], eps, alpha, steps, clip, seed, first_row=off))
    return np.concatenate(out)


# ---- 1. the start -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", TWINS)
def test_the_start_is_the_definition(gnn, oracle_mod, name, dtype):
    c = ac.BY_NAME[name]
    X, Y = ac.rows(c)
    Xh, Yh = ac.held_rows(c)
    net = make_net(gnn, oracle_mod, c, dtype)
    net.upload_dataset(X, Y)
    net.upload_held_out(Xh, Yh)
    for seed in (0, pc.START_SEED, 2 ** 31 - 1):
        a0 = net.pgd_range(pc.EPS, pc.ALPHA, 0, start_seed=seed)
        assert a0.shape == X.shape and a0.dtype == np.float64
        assert same_bits(a0, pc.start(X, seed, np.arange(c.n))), (name, seed)
    assert np.array_equal(net.pgd_range(pc.EPS, pc.ALPHA, 0, start_seed=pc.START_SEED), pc.start(X, pc.START_SEED, np.arange(c.n)))
    if c.n > 8:     # a range that starts inside the set: the key is the row's index in the set, over every block
        first = 3
        got = net.pgd_range(pc.EPS, pc.ALPHA, 0, first, c.n - first, start_seed=pc.START_SEED)
        assert same_bits(got, pc.start(X[first:], pc.START_SEED, first + np.arange(c.n - first)))
        assert same_bits(got, pc.start_buffer(X[first:], pc.START_SEED, first, c.max_batch))
    clip = pc.FAULT_CLIP                        # lo > 0, rows outside the box
    assert same_bits(net.pgd_range(pc.EPS, pc.ALPHA, 0, clip=clip, start_seed=pc.START_SEED), pc.start(X, pc.START_SEED, np.arange(c.n), clip=clip))
    assert same_bits(net.pgd_range(pc.EPS, pc.ALPHA, 0, held_out=True, start_seed=pc.START_SEED), pc.start(Xh, pc.START_SEED, np.arange(c.n)))
    # no seed, no steps: the rows, clipped to the box
    assert same_bits(net.pgd_range(pc.EPS, pc.ALPHA, 0), X)
    assert same_bits(net.pgd_range(pc.EPS, pc.ALPHA, 0, clip=clip), np.clip(X.astype(np.float32), pc.f32(clip[0]), pc.f32(clip[1])))
    assert same_bits(net.pgd_range(0.0, pc.ALPHA, 0, start_seed=pc.START_SEED), X)      # eps = 0: the ball is the row


# ---- 2. one step of size eps is FGSM ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", TWINS)
def test_one_step_of_size_eps_is_fgsm(gnn, oracle_mod, name, dtype):
    c = ac.BY_NAME[name]
    X, Y = ac.rows(c)
    Xh, Yh = ac.held_rows(c)
    net = make_net(gnn, oracle_mod, c, dtype)
    net.upload_dataset(X, Y)
    net.upload_held_out(Xh, Yh)
    for eps in ac.EPS:
        for clip in (pc.CLIP, pc.FAULT_CLIP):
            assert same_bits(net.pgd_range(eps, eps, 1, clip=clip), net.fgsm_range(eps, clip=clip)), (name, eps, clip)
            h, l = net.evaluate_pgd_range(eps, eps, 1, clip=clip)
            hf, lf = net.evaluate_fgsm_range(eps, clip=clip)
            assert h == hf and bits(l) == bits(lf)
    assert same_bits(net.pgd_range(0.1, 0.1, 1, held_out=True), net.fgsm_range(0.1, held_out=True))
    h, l = net.evaluate_pgd_range(0.1, 0.1, 1, held_out=True)
    hf, lf = net.evaluate_fgsm_range(0.1, held_out=True)
    assert h == hf and bits(l) == bits(lf)
    if c.n > 8:
        assert same_bits(net.pgd_range(0.1, 0.1, 1, 3, c.n - 5), net.fgsm_range(0.1, 3, c.n - 5))


# ---- 3. the host route, bit for bit --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name,dtype", TWINS)
def test_rows_are_the_host_route(gnn, oracle_mod, name, dtype, seed):
    c = ac.BY_NAME[name]
    X, Y = ac.rows(c)
    net = make_net(gnn, oracle_mod, c, dtype)
    net.upload_dataset(X, Y)
    adv = net.pgd_range(pc.EPS, pc.ALPHA, pc.T, start_seed=seed)
    assert adv.shape == X.shape and adv.dtype == np.float64
    want = host_route(gnn, net, X, Y, 0, c.n, c.max_batch, seed=seed)
    assert same_bits(adv, want), (name, seed, int((adv != want).sum()))
    assert np.array_equal(net.pgd_range(pc.EPS, pc.ALPHA, pc.T, 0, c.n, start_seed=seed), adv)      # the same bits every time
    assert (np.abs(adv - X).max() > 0.09) and not same_bits(adv, net.fgsm_range(pc.EPS))
    if c.n > 8:                                                   # a range that starts inside the set
        got = net.pgd_range(pc.EPS, pc.ALPHA, pc.T, 3, c.n - 5, start_seed=seed)
        assert same_bits(got, host_route(gnn, net, X, Y, 3, c.n - 5, c.max_batch, seed=seed))
    clip = pc.FAULT_CLIP                                          # lo > 0, rows outside the box
    assert same_bits(net.pgd_range(pc.EPS, pc.ALPHA, pc.T, clip=clip, start_seed=seed),
                     host_route(gnn, net, X, Y, 0, c.n, c.max_batch, clip=clip, seed=seed))
    if seed is None and c.inner == ac.RELU:                       # g == 0 exactly at every step: the pixel stays 0
        assert np.all(adv[X == 0.0] == 0.0) and (X == 0.0).mean() > 0.4


@pytest.mark.parametrize("name,dtype", [("relu_zeros", F32), ("blocks", F32), ("blocks_dense", BF16), ("per_layer", F32), ("gemm_plan", BF16)])
def test_rows_of_the_held_out_set(gnn, oracle_mod, name, dtype):
    """the held-out rows attacked as a net of the same weights attacks them as ITS training set; the training set's results are
    not disturbed"""
    c = ac.BY_NAME[name]
    X, Y = ac.rows(c)
    Xh, Yh = ac.held_rows(c)
    net, twin = make_net(gnn, oracle_mod, c, dtype), make_net(gnn, oracle_mod, c, dtype)
    net.upload_dataset(X, Y)
    net.upload_held_out(Xh, Yh)
    twin.upload_dataset(Xh, Yh)
    for seed in SEEDS:
        before = net.pgd_range(pc.EPS, pc.ALPHA, pc.T, start_seed=seed)
        adv = net.pgd_range(pc.EPS, pc.ALPHA, pc.T, held_out=True, start_seed=seed)
        assert same_bits(adv, twin.pgd_range(pc.EPS, pc.ALPHA, pc.T, start_seed=seed))
        assert same_bits(adv, host_route(gnn, net, Xh, Yh, 0, c.n, c.max_batch, seed=seed))
        assert net.evaluate_pgd_range(pc.EPS, pc.ALPHA, pc.T, held_out=True, start_seed=seed) == twin.evaluate_pgd_range(pc.EPS, pc.ALPHA, pc.T, start_seed=seed)
        assert np.array_equal(net.pgd_range(pc.EPS, pc.ALPHA, pc.T, start_seed=seed), before)


# ---- 4. the fp64 model, teacher-forced ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", MODEL)
def test_every_step_is_the_models_step_from_the_device_iterate(gnn, oracle_mod, name, dtype):
    c = ac.BY_NAME[name]
    bf = dtype == BF16
    X, Y = ac.rows(c)
    Ws = ac.weights(oracle_mod, c)
    net = make_net(gnn, oracle_mod, c, dtype)
    net.upload_dataset(X, Y)
    lo, hi = pc.feasible(X)
    x = net.pgd_range(pc.EPS, pc.ALPHA, 0)
    assert same_bits(x, X)
    for t in range(pc.T):
        nxt = net.pgd_range(pc.EPS, pc.ALPHA, t + 1)
        g = ac.gradient(Ws, x, Y, c.inner, bf)
        dec = ac.decided(g, x, c.inner, bf)
        want = pc.step(x, X, g).astype(np.float32)
        got = nxt.astype(np.float32)
        off = got != want
        allowed = [pc.step(x, X, g, dtype=np.float32, s=np.full(X.shape, s)) for s in (-1.0, 0.0, 1.0)]
        one_of = (got == allowed[0]) | (got == allowed[1]) | (got == allowed[2])
        print("%s %s step %d: %d of %d elements undecided, %d of them off the model; %d decided elements off"
              % (name, "bf16" if bf else "f32", t + 1, (~dec).sum(), dec.size, (off & ~dec).sum(), (off & dec).sum()))
        assert not (off & dec).any()
        assert one_of.all()
        assert (~dec).mean() <= ac.UNDECIDED_CAP
        assert np.all(got >= lo) and np.all(got <= hi)
        x = nxt
    edge = (got == X.astype(np.float32) - pc.f32(pc.EPS)) | (got == X.astype(np.float32) + pc.f32(pc.EPS))
    assert edge.mean() > 0.25       # the projection acted


# ---- 5. evaluation ------------------------------------------------------------------------------------------------------------------
def _host_evaluation(net, adv, Y, mb):
    """hits and the fp64 per-row losses of the rows fed back as host batches, block by block"""
    hits, losses = 0, []
    e = expected_rule(Y)
    for off in range(0, len(adv), mb):
        rows = slice(off, min(off + mb, len(adv)))
        hits += int((net.argmax(adv[rows]) == e[rows]).sum())
        losses.append(np.atleast_1d(net.calculateLoss(adv[rows], Y[rows])))
    return hits, np.concatenate(losses)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name,dtype", TWINS)
def test_robust_hits_loss_and_curve(gnn, oracle_mod, name, dtype, seed):
    c = ac.BY_NAME[name]
    X, Y = ac.rows(c)
    net = make_net(gnn, oracle_mod, c, dtype)
    net.upload_dataset(X, Y)
    net.train_range(0, min(c.n, c.max_batch), 30, 0.05, 0.9)       # briefly trained: the hits are neither none nor all
    kw = dict(start_seed=seed)
    hits, loss = net.evaluate_pgd_range(pc.EPS, pc.ALPHA, pc.T, 0, c.n, **kw)
    assert (hits, loss) == net.evaluate_pgd_range(pc.EPS, pc.ALPHA, pc.T, **kw)            # the same bits every time
    adv = net.pgd_range(pc.EPS, pc.ALPHA, pc.T, **kw)
    want_hits, rows_loss = _host_evaluation(net, adv, Y, c.max_batch)
    bound = (1e-4 * np.abs(rows_loss) + 1e-5).sum()
    print("%s %d seed %s: hits %d of %d (clean %d), loss sum %.9g against %.9g (off by %.3g, budget %.3g)"
          % (name, dtype, seed, hits, c.n, net.count_hits_range(0, c.n), loss, rows_loss.sum(), abs(loss - rows_loss.sum()), bound))
    assert hits == want_hits
    assert abs(loss - rows_loss.sum()) <= bound
    # the curve: entry t is the call with t steps, in both bits
    ch, cl = net.evaluate_pgd_range(pc.EPS, pc.ALPHA, pc.T, curve=True, **kw)
    assert ch.shape == (pc.T + 1,) and cl.shape == (pc.T + 1,) and ch.dtype == np.int64
    for t in range(pc.T + 1):
        h, l = net.evaluate_pgd_range(pc.EPS, pc.ALPHA, t, **kw)
        assert int(ch[t]) == h and bits(cl[t]) == bits(l), (t, ch, cl, h, l)
    if seed is None:                                                   # entry 0 is the rows themselves
        assert int(ch[0]) == net.count_hits_range(0, c.n)
        assert abs(cl[0] - net.evaluate_range(0, c.n)[1]) <= bound
        if c.n >= 16:                                                  # (the one-row net, trained on its row, has loss 0.0 either way)
            assert cl[-1] > cl[0]                                      # the attack raises the loss
    if c.n > 8:
        part = net.evaluate_pgd_range(pc.EPS, pc.ALPHA, pc.T, 3, c.n - 5, curve=True, **kw)
        one = net.evaluate_pgd_range(pc.EPS, pc.ALPHA, pc.T, 3, c.n - 5, **kw)
        assert int(part[0][-1]) == one[0] and bits(part[1][-1]) == bits(one[1])


def _state(net):
    return net.get_weights(), net.get_momentum(), net.time


def _same_state(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


# ---- 7. nothing moves -----------------------------------------------------------------------------------------------------------------
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
    e, a, T = pc.EPS, pc.ALPHA, pc.T

    def run(ask):
        net = make_net(gnn, oracle_mod, c, dtype, max_batch=B)
        assert net.step_launches == launches, net.plan_note
        net.upload_dataset(X, Y)
        net.upload_held_out(X[:20], Y[:20])
        out = []
        net.train_range(0, B, 5, 0.05, 0.9)
        if ask:
            before = _state(net)
            net.evaluate_pgd_range(e, a, T, 0, n)
            net.pgd_range(e, a, 1, 0, n)
            net.pgd_range(e, a, T, 0, n, start_seed=3)
            _same_state(before, _state(net))
        net.train_range(5 * B, B, 5, 0.05, 0.9)
        out.append(_state(net))
        net.gradientStep(X[:B], 0.05, 0.9, False, expected=Y[:B])
        if ask:
            net.pgd_range(e, a, T, B, 2 * B + 3)
            net.evaluate_pgd_range(e, a, T, held_out=True, curve=True)
        net.gradientStep(X[B:2 * B], 0.05, 0.9, False, expected=Y[B:2 * B])
        out.append(_state(net))
        smp = gnn.Sampler(n, seed=3)
        net.train_sampled(smp, 6, B, 0.05, 0.9)
        if ask:
            net.evaluate_pgd_range(e, a, T, 5, n - 5, start_seed=1, curve=True)
            net.pgd_range(e, a, 0, held_out=True)
            net.pgd_range(e, a, 1, 0, 2 * B)
        net.train_sampled(smp, 6, B, 0.05, 0.9)
        out.append(_state(net))
        out.append(smp.sample(B))
        return out

    with_calls, without = run(True), run(False)
    assert without[0][2] == 10 and without[2][2] == 24
    for x, y in zip(with_calls[:3], without[:3]):
        _same_state(x, y)
    assert np.array_equal(with_calls[3], without[3])


# ---- 6. training ------------------------------------------------------------------------------------------------------------------------
def _train_net(gnn, t, dtype):
    return gnn.SoftmaxCrossEntropyNeuralNet(t.dims, inner_act=t.inner, seed=t.seed, dtype=dtype, max_batch=t.batch)


# (the second clip, with lo > 0, on the batch-8 fixtures: a padding cell that went through the formula would become lo)
TRAIN_TWINS = [(t.name, dt, clip, seed) for t in ac.TWIN_RUNS for dt in (F32, BF16) for clip in (pc.CLIP, pc.FAULT_CLIP) for seed in SEEDS
               if clip == pc.CLIP or (t.batch == 8 and seed is not None)]


@pytest.mark.parametrize("run,dtype,clip,seed", TRAIN_TWINS)
def test_training_is_the_host_driven_loop(gnn, run, dtype, clip, seed):
    """40 iterations of gnn_mlp_train_sampled_pgd against: an identical Sampler, and per iteration gnn_amd.pgd on the drawn rows --
    the start keyed by the drawn dataset indices and the iteration's number -- then gradientStep: weights, momentum, time and the
    sampler's state bit for bit."""
    t = [r for r in ac.TWIN_RUNS if r.name == run][0]
    X, Y = ac.train_rows(t)
    step, momentum = ac.TRAIN_HYPER
    net, twin = _train_net(gnn, t, dtype), _train_net(gnn, t, dtype)
    if dtype == F32:
        assert net.step_launches == (2 if run.startswith("two_launch") else 0), net.plan_note
    net.upload_dataset(X, Y)
    smp, smp2 = gnn.Sampler(t.n_rows, seed=ac.SAMPLER_SEED), gnn.Sampler(t.n_rows, seed=ac.SAMPLER_SEED)
    net.train_sampled_pgd(smp, pc.TRAIN_ITERATIONS, t.batch, step, momentum, ac.TRAIN_EPS, pc.TRAIN_ALPHA, pc.TRAIN_T, clip, seed)
    drawn = 0
    for i in range(pc.TRAIN_ITERATIONS):
        idx = smp2.sample(t.batch)
        drawn += len(idx)
        adv = gnn.pgd(twin, X[idx], Y[idx], ac.TRAIN_EPS, pc.TRAIN_ALPHA, pc.TRAIN_T, clip, seed, first_row=idx, iteration=i)
        twin.gradientStep(adv, step, momentum, False, expected=Y[idx])
    assert drawn > t.n_rows or t.batch * pc.TRAIN_ITERATIONS <= t.n_rows
    _same_state(_state(net), _state(twin))
    assert net.time == pc.TRAIN_ITERATIONS
    assert np.abs(net.get_weights() - _train_net(gnn, t, dtype).get_weights()).max() > 1e-3    # (it trained)
    for _ in range(3):      # the handle's sampler stands where the twin's stands
        assert np.array_equal(smp.sample(t.batch), smp2.sample(t.batch))


def test_the_sampler_ends_where_train_sampled_leaves_it(gnn):
    t = ac.TWIN_RUNS[0]
    X, Y = ac.train_rows(t)
    step, momentum = ac.TRAIN_HYPER
    a, b = _train_net(gnn, t, F32), _train_net(gnn, t, F32)
    a.upload_dataset(X, Y)
    b.upload_dataset(X, Y)
    sa, sb = gnn.Sampler(t.n_rows, seed=ac.SAMPLER_SEED), gnn.Sampler(t.n_rows, seed=ac.SAMPLER_SEED)
    a.train_sampled_pgd(sa, pc.TRAIN_ITERATIONS, t.batch, step, momentum, ac.TRAIN_EPS, pc.TRAIN_ALPHA, pc.TRAIN_T, start_seed=1)
    b.train_sampled(sb, pc.TRAIN_ITERATIONS, t.batch, step, momentum)
    assert a.time == b.time == pc.TRAIN_ITERATIONS
    for _ in range(3):
        assert np.array_equal(sa.sample(t.batch), sb.sample(t.batch))


def test_training_follows_the_oracle(gnn, oracle_mod):
    """the run tests/test_pgd_cpu.py::test_the_oracle_run_meets_no_undecided_element holds free of undecided elements"""
    t = pc.ORACLE_RUN
    X, Y = ac.train_rows(t)
    step, momentum = ac.TRAIN_HYPER
    w0 = ac.reference_net(oracle_mod, t.dims, t.inner, t.seed).get_weights()
    w, v, _ = pc.train_model(w0, t, X, Y, ac.draws(gnn, t, pc.ORACLE_ITERATIONS))
    net = _train_net(gnn, t, F32)
    assert np.abs(net.get_weights() - w0).max() <= 1e-7
    net.upload_dataset(X, Y)
    smp = gnn.Sampler(t.n_rows, seed=ac.SAMPLER_SEED)
    net.train_sampled_pgd(smp, pc.ORACLE_ITERATIONS, t.batch, step, momentum, ac.TRAIN_EPS, pc.TRAIN_ALPHA, pc.TRAIN_T)
    bud = ac.W_ATOL * pc.ORACLE_ITERATIONS
    dw, dv = np.abs(net.get_weights() - w).max(), np.abs(net.get_momentum() - v).max()
    print("oracle run: dw %.3g dv %.3g of the budget %.3g" % (dw / bud, dv / bud, bud))
    assert dw <= bud and dv <= bud


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------
def _refused(gnn, code, fn):
    with pytest.raises(gnn.GnnError) as e:
        fn()
    assert e.value.code == code, (e.value.code, str(e.value))
    return str(e.value)


def test_refusals_leave_the_net_alone(gnn, oracle_mod):
    c = ac.BY_NAME["ident"]
    X, Y = ac.rows(c)
    capi = gnn._capi
    e, a, T = pc.EPS, pc.ALPHA, pc.T
    for inner in (ac.SIGMOID, ac.TANH):     # the device holds f(x), not x
        net = gnn.SoftmaxCrossEntropyNeuralNet(c.dims, inner_act=inner, max_batch=c.n)
        net.upload_dataset(X, Y)
        smp = gnn.Sampler(c.n, seed=1)
        before = _state(net)
        for fn in (lambda: net.pgd_range(e, a, T), lambda: net.evaluate_pgd_range(e, a, T),
                   lambda: net.train_sampled_pgd(smp, 3, 8, 0.05, 0.9, e, a, T)):
            assert "f(x)" in _refused(gnn, capi.ERR_UNSUPPORTED, fn)
        _same_state(before, _state(net))
        assert np.array_equal(smp.sample(8), gnn.Sampler(c.n, seed=1).sample(8))     # (no draw was taken)
    net, twin = make_net(gnn, oracle_mod, c), make_net(gnn, oracle_mod, c)
    smp = gnn.Sampler(c.n, seed=1)
    for fn in (lambda: net.pgd_range(e, a, T, 0, 4), lambda: net.evaluate_pgd_range(e, a, T, 0, 4),
               lambda: net.train_sampled_pgd(smp, 3, 8, 0.05, 0.9, e, a, T),
               lambda: net.pgd_range(e, a, T, 0, 4, held_out=True), lambda: net.evaluate_pgd_range(e, a, T, 0, 4, held_out=True)):
        _refused(gnn, capi.ERR_STATE, fn)       # no data set uploaded
    net.upload_dataset(X, Y)
    twin.upload_dataset(X, Y)
    # every refusal below stands behind a host-batch step whose update is still pending: it is applied, nothing else happens
    for n_ in (net, twin):
        n_.gradientStep(X[:8], 0.05, 0.9, False, expected=Y[:8])
    bad = [dict(eps=-0.1), dict(eps=float("inf")), dict(eps=float("nan")), dict(clip=(-0.1, 1.0)), dict(clip=(0.5, 0.25)),
           dict(clip=(float("nan"), 1.0)), dict(clip=(0.0, float("nan"))),
           dict(alpha=-0.01), dict(alpha=float("inf")), dict(alpha=float("nan")), dict(steps=-1), dict(steps=1025),
           dict(seed=2 ** 31), dict(seed=2 ** 40)]
    for kw in bad:
        p = dict(eps=e, alpha=a, steps=T, clip=(0.0, 1.0), seed=None)
        p.update(kw)
        _refused(gnn, capi.ERR_BAD_ARG, lambda: net.pgd_range(p["eps"], p["alpha"], p["steps"], 0, 4, clip=p["clip"], start_seed=p["seed"]))
        _refused(gnn, capi.ERR_BAD_ARG, lambda: net.evaluate_pgd_range(p["eps"], p["alpha"], p["steps"], 0, 4, clip=p["clip"], start_seed=p["seed"]))
        _refused(gnn, capi.ERR_BAD_ARG, lambda: net.evaluate_pgd_range(p["eps"], p["alpha"], p["steps"], 0, 4, clip=p["clip"], start_seed=p["seed"], curve=True))
        _refused(gnn, capi.ERR_BAD_ARG, lambda: net.train_sampled_pgd(smp, 3, 8, 0.05, 0.9, p["eps"], p["alpha"], p["steps"], p["clip"], p["seed"]))
        net.gradientStep(X[8:16], 0.05, 0.9, False, expected=Y[8:16])       # (a pending update in front of the next refusal)
        twin.gradientStep(X[8:16], 0.05, 0.9, False, expected=Y[8:16])
    # the limits themselves are served
    assert net.pgd_range(e, 0.0, 2, 0, 4).shape == (4, c.dims[0])
    assert same_bits(net.pgd_range(e, a, 0, 0, 4, start_seed=2 ** 31 - 1), pc.start(X[:4], 2 ** 31 - 1, np.arange(4)))
    for first, n in ((0, c.n + 1), (-1, 2), (c.n, 1), (0, 0)):      # rows outside the set
        _refused(gnn, capi.ERR_BAD_ARG, lambda: net.pgd_range(e, a, T, first, n))
        _refused(gnn, capi.ERR_BAD_ARG, lambda: net.evaluate_pgd_range(e, a, T, first, n))
    _refused(gnn, capi.ERR_STATE, lambda: net.pgd_range(e, a, T, 0, 4, held_out=True))      # no held-out set
    import ctypes as C
    out = np.empty((4, c.dims[0]))
    dp = out.ctypes.data_as(C.POINTER(C.c_double))
    _refused(gnn, capi.ERR_BAD_ARG, lambda: capi.check(net._lib.gnn_mlp_pgd_set_range(net._h, 2, 0, 4, e, a, T, -1, 0.0, 1.0, dp)))   # a set that is neither
    _refused(gnn, capi.ERR_BAD_ARG, lambda: capi.check(net._lib.gnn_mlp_pgd_set_range(net._h, 0, 0, 4, e, a, T, -1, 0.0, 1.0, None)))
    _refused(gnn, capi.ERR_BAD_ARG, lambda: capi.check(net._lib.gnn_mlp_evaluate_pgd_set_range(net._h, 0, 0, 4, e, a, T, -1, 0.0, 1.0, 0, None, None)))
    hits = C.c_int64()
    _refused(gnn, capi.ERR_BAD_ARG, lambda: capi.check(net._lib.gnn_mlp_evaluate_pgd_set_range(net._h, 0, 0, 4, e, a, T, -1, 0.0, 1.0, 2, C.byref(hits), None)))
    # what gnn_mlp_train_sampled refuses: a batch that is the whole set, no iterations, a sampler of another size
    _refused(gnn, capi.ERR_BAD_ARG, lambda: net.train_sampled_pgd(smp, 3, c.n, 0.05, 0.9, e, a, T))
    _refused(gnn, capi.ERR_BAD_ARG, lambda: net.train_sampled_pgd(smp, 0, 8, 0.05, 0.9, e, a, T))
    _refused(gnn, capi.ERR_BAD_ARG, lambda: net.train_sampled_pgd(gnn.Sampler(c.n + 1, seed=1), 3, 8, 0.05, 0.9, e, a, T))
    _same_state(_state(twin), _state(net))
    assert net.time == 1 + len(bad)
    assert np.array_equal(smp.sample(8), gnn.Sampler(c.n, seed=1).sample(8))
    # members of a group are out of scope
    grp = gnn.NetGroup(c.dims, [1, 2], inner_act=c.inner, max_batch=c.n)
    grp.upload_dataset(X, Y)
    _refused(gnn, capi.ERR_STATE, lambda: grp.members[0].pgd_range(e, a, T, 0, 4))
    _refused(gnn, capi.ERR_STATE, lambda: grp.members[0].evaluate_pgd_range(e, a, T, 0, 4))
