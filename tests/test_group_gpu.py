"""NetGroup (gnn_mlp_group_*): K nets of one shape trained side by side.  Member k after any group call must be bit for bit
the lone handle created with seeds[k] that made the same calls with steps[k], momenta[k] -- weights, momentum and time."""
import ctypes as C

import os

import numpy as np
import pytest

from tests import chain_cases as cc

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


# ---- the drawn cases of tests/chain_cases.py in groups --------------------------------------------------------------------------
# (seed, dtype, K).  Grouped launches exist where the row-block kernel applies (group.hip), i.e. on the even seeds; among them:
# both net classes (seeds 2, 14, 17, 20 are GeneralNeuralNets), 3 to 6 layers, the 1024-wide input (seed 6), nine batch sizes
# whose row of row-block workgroups is padded to a multiple of 8 in the grouped grid -- the workgroups behind member k's last
# live one return at once -- two of them with B <= 16 (seeds 0, 12), K = 16 three times (the whole GroupArgs arrays), bf16 in
# its three- and four-layer forms.
GROUPED_CASES = [(0, 0, 16), (6, 0, 5), (10, 0, 2), (12, 0, 5), (14, 0, 16), (16, 0, 2), (17, 0, 5), (20, 0, 2),
                 (2, 1, 5), (14, 1, 2), (18, 1, 16), (22, 1, 2)]
# Off the two-launch path -- 17 first-layer K slabs (seed 7, 1025 inputs) -- or on it without the row-block kernel (seed 13: 374
# hidden neurons in front of 30 outputs): the members are stepped one after another, the sampler rewound for each.
FALLBACK_CASES = [(7, 0, 2), (13, 0, 5)]
W_ATOL = 2e-6   # per step, f32 against the fp64 oracle (tests/test_trainer_gpu.py)


def _case_hyper(K):
    """Distinct per member, all near the cases' own 0.0125 / 0.9 (the oracle budget is the project's for steps of that size)."""
    return [cc.STEP * (1 + k / 32) for k in range(K)], [cc.MOMENTUM - 0.01 * k for k in range(K)]


def _case_lone(gnn, case, seed, dtype):
    dims, B, inner, out_kind, last = case
    if out_kind == cc.OUT_SOFTMAX_CE:
        return gnn.SoftmaxCrossEntropyNeuralNet(dims, inner_act=inner, seed=seed, dtype=dtype, max_batch=B)
    return gnn.GeneralNeuralNet(dims, inner_act=inner, last_act=last, seed=seed, dtype=dtype, max_batch=B)


def _group_case(gnn, oracle_mod, seed, dtype, K, want_launches):
    if os.environ.get("GNN_MLP_PATH") or os.environ.get("GNN_MLP_CHAIN") == "0" or os.environ.get("GNN_MLP_ROWBLOCK") == "0":
        pytest.skip("path forced by the environment")
    case = cc.chain_case(seed)
    dims, B, inner, out_kind, last = case
    N = cc.dataset_rows(B)
    X, Y = cc.chain_data(seed, dims, B)
    Xs, Ys = X[B:2 * B], Y[B:2 * B]                      # the host batch of the lone steps
    steps, moms = _case_hyper(K)
    seeds = list(range(1, K + 1))
    g = gnn.NetGroup(dims, seeds, out_kind=out_kind, inner_act=inner, last_act=last if out_kind == cc.OUT_ACT_LOSS else gnn.ACT_IDENTITY,
                     dtype=dtype, max_batch=B)
    probe = _case_lone(gnn, case, 1, dtype)
    print("group-case seed %d dims %s B %d dtype %d K %d grid %d | group launches %d, lone launches %d rowblock %d note %r"
          % (seed, "-".join(map(str, dims)), B, dtype, K, cc.rowblock_grid(B), g.launches_per_step, probe.step_launches,
             probe.rowblock_state, probe.plan_note))
    probe.close()
    assert g.launches_per_step == want_launches
    w0 = [m.get_weights() * cc.W_SCALE for m in g.members]
    for m, w in zip(g.members, w0):
        m.set_weights(w)
    g.upload_dataset(X, Y)

    def calls(train_sampled, train_range, lone_step):
        """The case's calls; between the two calls of each loop member 0 alone takes a step on a host batch, so that the group
        finds its members' look-ahead states unequal (enter_grouped) and drops them."""
        train_sampled(17); lone_step(); train_sampled(7)
        train_range(0, 9); lone_step(); train_range(2 * B, 8)

    s = gnn.Sampler(N, seed=cc.SAMPLER_SEED)
    calls(lambda n: g.train_sampled(s, n, B, steps, moms),
          lambda first, n: g.train_range(first, B, n, steps, moms),
          lambda: g.members[0].gradientStep(Xs, 0.02, 0.8, False, expected=Ys))
    for k in range(K):
        lone = _case_lone(gnn, case, seeds[k], dtype)
        lone.set_weights(w0[k])
        lone.upload_dataset(X, Y)
        ls = gnn.Sampler(N, seed=cc.SAMPLER_SEED)

        def sampled(n):
            assert lone._lib.gnn_mlp_train_sampled(lone._h, ls._h, n, B, steps[k], moms[k], 0) == 0
        calls(sampled, lambda first, n: lone.train_range(first, B, n, steps[k], moms[k]),
              (lambda: lone.gradientStep(Xs, 0.02, 0.8, False, expected=Ys)) if k == 0 else (lambda: None))
        _assert_same(g.members[k], lone, "(seed %d, member %d of %d)" % (seed, k, K))
        assert lone.time == 41 + 2 * (k == 0)
        if k == K - 1:      # the shared sampler ends where a lone one ends: advanced by one call's draws, not once per member
            assert np.array_equal(s.sample(B), ls.sample(B))
        lone.close(); ls.close()
    if dtype == 0:
        # the last member against the fp64 oracle on the same batches (a group of wrong-but-equal nets would pass the above)
        k = K - 1
        ref = oracle_mod.OracleNet(dims, out_kind=out_kind, inner_act=inner, last_act=last)
        ref.set_alloc_per_sample(0)
        ref.set_weights(w0[k])
        for idx in cc.sampled_draws(oracle_mod, N, B):
            ref.gradient_step(X[idx], Y[idx], steps[k], moms[k])
        for first, n in ((0, 9), (2 * B, 8)):
            for r in cc.range_batches(N, B, first, n):
                ref.gradient_step(X[r:r + B], Y[r:r + B], steps[k], moms[k])
        assert ref.time == g.members[k].time == 41
        dw = np.abs(g.members[k].get_weights() - ref.get_weights()).max()
        dv = np.abs(g.members[k].get_momentum() - ref.get_momentum()).max()
        print("group-case seed %d member %d against the oracle: dw %.3f dv %.3f of the budget" % (seed, k, dw / (W_ATOL * 41), dv / (W_ATOL * 41)))
        assert dw <= W_ATOL * 41 and dv <= W_ATOL * 41, (case, K, dw, dv)
    s.close()
    g.close()


@pytest.mark.parametrize("seed,dtype,K", GROUPED_CASES, ids=["seed%d-%s-K%d" % (s, "bf16" if d else "f32", k) for s, d, k in GROUPED_CASES])
def test_drawn_cases_in_grouped_launches(gnn, oracle_mod, seed, dtype, K):
    """train_sampled (17 + 7 draws of one shared sampler, batches shortened at a refill) and train_range (two calls, wrapping) of
    a group against lone handles making the same calls -- bitwise, every member -- at drawn shapes: the runtime-shape grouped
    instances for every layer count and both classes, ragged batches, ragged input widths."""
    _group_case(gnn, oracle_mod, seed, dtype, K, 2)


@pytest.mark.parametrize("seed,dtype,K", FALLBACK_CASES, ids=["seed%d-K%d" % (s, k) for s, _, k in FALLBACK_CASES])
def test_drawn_cases_member_after_member(gnn, oracle_mod, seed, dtype, K):
    """The same calls where a group has no grouped launches: gnn_mlp_group_train_sampled hands every member the sampler in its
    state at the call (sampler_copy / sampler_assign) and leaves it advanced once."""
    _group_case(gnn, oracle_mod, seed, dtype, K, 0)


def test_the_group_cases_cover_what_they_are_chosen_for():
    cases = {(s, d): cc.chain_case(s) for s, d, _ in GROUPED_CASES}
    assert {c[3] for c in cases.values()} == {cc.OUT_SOFTMAX_CE, cc.OUT_ACT_LOSS}
    assert {len(c[0]) for (s, d), c in cases.items() if d == 0} == {3, 4, 5, 6}
    assert {len(c[0]) for (s, d), c in cases.items() if d == 1} == {3, 4}
    ragged = {s for (s, d), c in cases.items() if cc.rowblock_grid(c[1]) % 8}
    assert len(ragged) >= 6 and any(cases[s, d][1] <= 16 for s, d in cases if s in ragged)
    assert 1024 in {c[0][0] for c in cases.values()} and cc.chain_case(FALLBACK_CASES[0][0])[0][0] == 1025
    assert sum(1 for _, _, k in GROUPED_CASES if k == 16) >= 3 and any(d == 1 and k == 16 for _, d, k in GROUPED_CASES)
    assert {k for _, _, k in GROUPED_CASES} == {2, 5, 16}
