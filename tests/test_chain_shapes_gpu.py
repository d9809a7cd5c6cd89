"""The resident-data training loops (gnn_mlp_train_sampled, gnn_mlp_train_range) on the drawn cases of tests/chain_cases.py.

Only these loops announce the next batch, so only they launch the look-ahead form of the tile-owner kernel
(tile_step_kernel<1,2,true>: weight gradient, momentum update and the NEXT batch's first-layer K slabs from the weights just
written), the row-block kernel's copy of the next batch's rows (RB_COPY_NEXT) and the index gather.  Per case, in f32 and bf16:

1. bitwise: the loop equals the same steps taken one call at a time (no look-ahead at all) -- weights, momentum, time;
2. f32: the sampled trajectory against the fp64 oracle driven by the oracle's own sampler, weights AND momentum within the
   project's 2e-6 per step (tests/test_trainer_gpu.py, tests/test_general_net_gpu.py) = 4.8e-5 after 24 steps.  What the budget
   catches was measured on the reference side (three wrong ORACLE trajectories on these 24 cases: a shortened batch divided
   by the nominal B; the last row of a ragged 4-row block dropped; the first-layer product taken from the weights before the
   previous update -- outside the budget in 24, 24 and 20 of the 24 cases, while a float32 numpy restatement of the correct
   trajectory stays within 1.6e-7 of the oracle);
3. bf16: against the bf16-aware numpy oracle after 3 and after 5 sampled steps (2e-4 / 4e-4, the bounds of
   test_general_net_bf16_against_bf16_oracle); the remaining steps are held by 1 alone;
4. f32: loss_range / argmax_range on resident rows after the trajectory, a ragged row count among them;
5. the same look-ahead from a caller's own loop (gnn_mlp_hint_next_range): announced batches of any start row and size, some
   announcements wrong -- bitwise against unannounced steps, f32 also against the oracle;
6. the kernels each case ran on (step_launches, rowblock_state, plan_note), with floors on how many cases take the
   two-launch path and each of its row kernels: the sweep cannot drift off the kernels it is for.

A lone handle instantiates its row kernels for its shape (hiprtc) at its 16th gradient computation, so the 24 steps also cross
from the runtime-shape kernels to the instantiated ones."""
import os

import numpy as np
import pytest

from tests import chain_cases as cc
from tests import np_oracle

pytestmark = pytest.mark.gpu

W_ATOL = 2e-6            # per step, weights and momentum (f32 against fp64)
SLAB_NOTE = "more than 16 first-layer K slabs"
SPLIT = (17, 7)          # the 24 sampled iterations in two calls: the first ends one draw into the sampler's second chunk
RANGE_CALLS = ((0, 9), (2, 8))   # (first batch, steps): five resident batches, both walks wrap


def _forced_path():
    e = os.environ
    return bool(e.get("GNN_MLP_PATH") or e.get("GNN_MLP_CHAIN") == "0" or e.get("GNN_MLP_ROWBLOCK") == "0" or e.get("GNN_MLP_JIT") == "0")


def _make(gnn, case, dtype, w0, X, Y):
    dims, B, inner, out_kind, last = case
    if out_kind == cc.OUT_SOFTMAX_CE:
        net = gnn.SoftmaxCrossEntropyNeuralNet(dims, inner_act=inner, dtype=dtype, max_batch=B)
    else:
        net = gnn.GeneralNeuralNet(dims, inner_act=inner, last_act=last, dtype=dtype, max_batch=B)
    net.set_weights(w0)
    net.upload_dataset(X, Y)
    return net


def _train_sampled(net, sampler, n, B):
    rc = net._lib.gnn_mlp_train_sampled(net._h, sampler._h, n, B, cc.STEP, cc.MOMENTUM, 0)
    assert rc == 0, rc


def _path(net):
    return net.step_launches, net.rowblock_state, net.plan_note


def _assert_bitwise(x, y, what):
    assert x.time == y.time, "time differs: " + what
    wx, wy = x.get_weights(), y.get_weights()
    if not np.array_equal(wx, wy):
        bad = np.flatnonzero(wx != wy)
        layer = [int(np.searchsorted(np.cumsum([a * b for a, b in zip(x.layer_dims[:-1], x.layer_dims[1:])]), i, side="right")) for i in bad[:4]]
        raise AssertionError("weights differ (%s): %d elements, max %.3g, first in layers %r" % (what, bad.size, np.abs(wx - wy).max(), layer))
    assert np.array_equal(x.get_momentum(), y.get_momentum()), "momentum differs: " + what


def _check_path_of_edge_widths(case, path):
    launches, _, note = path
    if case[0][0] == 1025:
        assert launches != 2 and SLAB_NOTE in note, path
    if case[0][0] in (1023, 1024):
        assert SLAB_NOTE not in note, path


@pytest.mark.parametrize("seed", range(cc.N_CASES))
def test_chained_loops_f32(gnn, oracle_mod, seed):
    if _forced_path():
        pytest.skip("path forced by the environment")
    case = cc.chain_case(seed)
    dims, B, inner, out_kind, last = case
    N = cc.dataset_rows(B)
    X, Y = cc.chain_data(seed, dims, B)
    ref, w0 = cc.oracle_net(oracle_mod, seed)
    a, b, c, d = (_make(gnn, case, gnn.DTYPE_F32, w0, X, Y) for _ in range(4))
    assert np.array_equal(a.get_weights(), w0)
    path0 = _path(a)
    _check_path_of_edge_widths(case, path0)

    # sampled: one loop in two calls against one indexed step per draw; the oracle on the oracle sampler's draws
    draws = cc.sampled_draws(oracle_mod, N, B)
    sa, sb = gnn.Sampler(N, seed=cc.SAMPLER_SEED), gnn.Sampler(N, seed=cc.SAMPLER_SEED)
    for n in SPLIT:
        _train_sampled(a, sa, n, B)
    for idx in draws:
        got = sb.sample(B)
        assert np.array_equal(got, idx), "product sampler and oracle sampler differ"
        b.gradient_step_indexed(got, cc.STEP, cc.MOMENTUM)
        ref.gradient_step(X[idx], Y[idx], cc.STEP, cc.MOMENTUM)
    assert np.array_equal(sa.sample(B), sb.sample(B)), "the loop left the sampler elsewhere"
    assert a.time == cc.ITERATIONS == ref.time
    path1 = _path(a)

    # contiguous: two calls that wrap against one range step per batch; the oracle on the same rows
    rows = [r for first, n in RANGE_CALLS for r in cc.range_batches(N, B, first * B, n)]
    for first, n in RANGE_CALLS:
        c.train_range(first * B, B, n, cc.STEP, cc.MOMENTUM)
    ref_c, _ = cc.oracle_net(oracle_mod, seed)
    for r in rows:
        d.gradient_step_range(r, B, cc.STEP, cc.MOMENTUM)
        ref_c.gradient_step(X[r:r + B], Y[r:r + B], cc.STEP, cc.MOMENTUM)

    dw = np.abs(a.get_weights() - ref.get_weights()).max()
    dv = np.abs(a.get_momentum() - ref.get_momentum()).max()
    dwc = np.abs(c.get_weights() - ref_c.get_weights()).max()
    dvc = np.abs(c.get_momentum() - ref_c.get_momentum()).max()
    budget, budget_c = W_ATOL * cc.ITERATIONS, W_ATOL * len(rows)
    print("chain-case f32 seed %d dims %s B %d act %d out %d/%d | launches %d rowblock %d->%d note %r | sampled dw %.3f dv %.3f  range dw %.3f dv %.3f of the budget"
          % (seed, "-".join(map(str, dims)), B, inner, out_kind, last, path0[0], path0[1], path1[1], path0[2],
             dw / budget, dv / budget, dwc / budget_c, dvc / budget_c))

    _assert_bitwise(a, b, "train_sampled against indexed steps, %r" % (path1,))
    _assert_bitwise(c, d, "train_range against range steps, %r" % (path1,))
    assert dw <= budget and dv <= budget, (case, path1, dw, dv)
    assert dwc <= budget_c and dvc <= budget_c, (case, path1, dwc, dvc)

    # evaluation of resident rows with the trained weights: a whole batch and the ragged remainder behind the five batches
    ref.set_weights(a.get_weights())
    for first, n in ((0, B), (5 * B, N - 5 * B)):
        Xr, Yr = X[first:first + n], Y[first:first + n]
        lr = ref.calculate_loss(Xr, Yr)
        assert np.all(np.abs(a.loss_range(first, n) - lr) <= 1e-4 * np.abs(lr) + 1e-5), (case, first, n)
        z = ref.logits(Xr) if out_kind == cc.OUT_SOFTMAX_CE else ref.propagate(Xr)
        s = np.sort(z, axis=1)
        safe = (s[:, -1] - s[:, -2]) > (1e-3 if out_kind == cc.OUT_SOFTMAX_CE else 1e-4)
        assert np.array_equal(a.argmax_range(first, n)[safe], ref.argmax(Xr)[safe]), (case, first, n)
    for net in (a, b, c, d):
        net.close()
    sa.close(); sb.close()


@pytest.mark.parametrize("seed", range(cc.N_CASES))
def test_chained_loops_bf16(gnn, oracle_mod, seed):
    if _forced_path():
        pytest.skip("path forced by the environment")
    case = cc.chain_case(seed)
    dims, B, inner, out_kind, last = case
    N = cc.dataset_rows(B)
    X, Y = cc.chain_data(seed, dims, B)
    X32 = X.astype(np.float32).astype(np.float64)      # inputs are f32 in HBM
    _, w0 = cc.oracle_net(oracle_mod, seed)
    a, b, c, d, e = (_make(gnn, case, gnn.DTYPE_BF16, w0, X, Y) for _ in range(5))
    path0 = _path(a)
    _check_path_of_edge_widths(case, path0)

    draws = cc.sampled_draws(oracle_mod, N, B)
    sa, sb, se = (gnn.Sampler(N, seed=cc.SAMPLER_SEED) for _ in range(3))
    for n in SPLIT:
        _train_sampled(a, sa, n, B)
    # the first 3 and 5 steps through the loop (e) against the bf16-aware oracle, and bitwise against the indexed steps (b)
    w, v = w0.copy(), np.zeros_like(w0)
    dev = {}
    for i, idx in enumerate(draws):
        got = sb.sample(B)
        assert np.array_equal(got, idx), "product sampler and oracle sampler differ"
        b.gradient_step_indexed(got, cc.STEP, cc.MOMENTUM)
        if i < 5:
            w, v = np_oracle.gradient_step_bf16(w, v, dims, X32[idx], Y[idx], cc.STEP, cc.MOMENTUM, inner, out_kind, last)
        if i in (2, 4):
            _train_sampled(e, se, 3 if i == 2 else 2, B)
            _assert_bitwise(e, b, "train_sampled against indexed steps after %d steps, %r" % (i + 1, path0))
            dev[i + 1] = (np.abs(e.get_weights() - w).max(), np.abs(e.get_momentum() - v).max())
    path1 = _path(a)

    rows = [r for first, n in RANGE_CALLS for r in cc.range_batches(N, B, first * B, n)]
    for first, n in RANGE_CALLS:
        c.train_range(first * B, B, n, cc.STEP, cc.MOMENTUM)
    for r in rows:
        d.gradient_step_range(r, B, cc.STEP, cc.MOMENTUM)

    print("chain-case bf16 seed %d dims %s B %d act %d out %d/%d | launches %d rowblock %d->%d note %r | after 3 steps dw %.3f dv %.3f of 2e-4, after 5 dw %.3f dv %.3f of 4e-4"
          % (seed, "-".join(map(str, dims)), B, inner, out_kind, last, path0[0], path0[1], path1[1], path0[2],
             dev[3][0] / 2e-4, dev[3][1] / 2e-4, dev[5][0] / 4e-4, dev[5][1] / 4e-4))

    assert a.time == cc.ITERATIONS
    _assert_bitwise(a, b, "train_sampled against indexed steps, %r" % (path1,))
    _assert_bitwise(c, d, "train_range against range steps, %r" % (path1,))
    assert dev[3][0] <= 2e-4 and dev[3][1] <= 2e-4, (case, path1, dev)
    assert dev[5][0] <= 4e-4 and dev[5][1] <= 4e-4, (case, path1, dev)
    for net in (a, b, c, d, e):
        net.close()
    for s in (sa, sb, se):
        s.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("seed", range(cc.N_CASES))
def test_announced_ranges_of_any_size(gnn, oracle_mod, seed, dtype):
    """gnn_mlp_hint_next_range as a caller uses it: resident batches that start at any row, some shorter than the one before
    (the tile kernel then makes the slabs of a batch of another size than the one whose gradient it forms -- in the loops above
    only sampled batches do that), two announcements of three right and one naming another batch.  Bitwise against the same
    range steps without announcements; f32 also against the oracle on the same rows."""
    if _forced_path():
        pytest.skip("path forced by the environment")
    case = cc.chain_case(seed)
    dims, B, inner, out_kind, last = case
    N = cc.dataset_rows(B)
    X, Y = cc.chain_data(seed, dims, B)
    ref, w0 = cc.oracle_net(oracle_mod, seed)
    dt = gnn.DTYPE_BF16 if dtype == "bf16" else gnn.DTYPE_F32
    hinted, plain = _make(gnn, case, dt, w0, X, Y), _make(gnn, case, dt, w0, X, Y)
    walk, hints = cc.hinted_walk(N, B)
    assert any(n < B for _, n in walk) and any(f % B for f, _ in walk) and any(h != w for h, w in zip(hints, walk[1:]))
    for s, (first, n) in enumerate(walk):
        if s < len(hints):
            hinted.hint_next_range(*hints[s])
        hinted.gradient_step_range(first, n, cc.STEP, cc.MOMENTUM)
        plain.gradient_step_range(first, n, cc.STEP, cc.MOMENTUM)
        if dtype == "f32":
            ref.gradient_step(X[first:first + n], Y[first:first + n], cc.STEP, cc.MOMENTUM)
    _assert_bitwise(hinted, plain, "announced against plain range steps, %r" % (_path(hinted),))
    if dtype == "f32":
        budget = W_ATOL * len(walk)
        dw = np.abs(hinted.get_weights() - ref.get_weights()).max()
        dv = np.abs(hinted.get_momentum() - ref.get_momentum()).max()
        print("chain-case hinted f32 seed %d: dw %.3f dv %.3f of the budget" % (seed, dw / budget, dv / budget))
        assert dw <= budget and dv <= budget, (case, _path(hinted), dw, dv)
    hinted.close(); plain.close()


def test_the_sweep_runs_on_the_kernels_it_is_for(gnn):
    """The floors of the sweep, read from fresh handles of every case (they are conditions on the draw, not measurements): at
    least 16 of the 24 f32 cases on the two-launch path; among the bf16 cases on it, the row-block kernel (three and four
    layers) and middle4_kernel (five and six layers) each at least twice; both f32 row kernels occur as well."""
    if _forced_path():
        pytest.skip("path forced by the environment")
    paths = {}
    for dtype in (gnn.DTYPE_F32, gnn.DTYPE_BF16):
        for seed in range(cc.N_CASES):
            dims, B, inner, out_kind, last = cc.chain_case(seed)
            net = (gnn.SoftmaxCrossEntropyNeuralNet(dims, inner_act=inner, dtype=dtype, max_batch=B) if out_kind == cc.OUT_SOFTMAX_CE
                   else gnn.GeneralNeuralNet(dims, inner_act=inner, last_act=last, dtype=dtype, max_batch=B))
            paths[dtype, seed] = (len(dims),) + _path(net)
            net.close()
    f32 = [paths[gnn.DTYPE_F32, s] for s in range(cc.N_CASES)]
    bf16 = [paths[gnn.DTYPE_BF16, s] for s in range(cc.N_CASES)]
    assert sum(1 for p in f32 if p[1] == 2) >= 16, f32
    assert sum(1 for p in f32 if p[1] == 2 and p[2] != 0) >= 2 and sum(1 for p in f32 if p[1] == 2 and p[2] == 0) >= 2, f32
    assert sum(1 for p in bf16 if p[1] == 2 and p[2] != 0 and p[0] in (3, 4)) >= 2, bf16
    assert sum(1 for p in bf16 if p[1] == 2 and p[2] == 0 and p[0] in (5, 6)) >= 2, bf16
    assert all(p[2] == 0 for p in bf16 if p[0] > 4), bf16       # (the bf16 row-block kernel: three and four layers)
