"""The data-parallel step inside the library (gnn_mlp_dp_*: csrc/dp.hip, csrc/dp_handle.h; the GSRC = 3 / 4 gradient sources of
tile_step_kernel and tile_step_bf16_kernel; direct_reduce_update_kernel, direct_reduce_scatter_kernel,
direct_gather_update_kernel) on the cases of tests/dp_cases.py: the 24 drawn nets of tests/chain_cases.py with 1 to 16
replicas that share device 0 in one process, and three hand-picked extras.  Per case, in f32 and bf16, for GNN_REDUCE_DIRECT and
GNN_REDUCE_DIRECT_RS:

a. bitwise: weights, momentum and time equal a reference built from the one-GPU hooks alone -- one lone handle per rank
   forms the partial gradient of its shard into a zeroed torch buffer (bind_grad_buffer, compute_gradient_range), torch adds
   the buffers in rank order (one IEEE f32 add each, like the kernels'), every rank applies the sum (apply_update).  Twice:
   without announcements (the flat update kernel) and with hint_next_range before every gradient (tile_step_kernel<2, 2, true>,
   which also puts the one-process-per-GPU hooks on these shapes).  sgd_adj is the update's one spelling, the sum is in rank
   order everywhere, look-ahead and hiprtc instantiation are bitwise-neutral: the bits must agree;
b. the walk (dp_cases.walk_calls): three train_range calls, two of which wrap over the five resident batches (successors
   announced: the fused reductions where the net takes the two-launch step), two gradient_step_range calls at rows that
   are no multiple of B (no announcement: the flat reducers), one host-batch gradientStep of resident rows; then a short
   tail -- a train_range of two steps and a host batch with FEWER ROWS THAN REPLICAS, so that replicas whose gradient buffer
   of the same parity holds a partial gradient now have no rows (a memset stands for their gradient, they get no
   announcement and update through the flat kernel next to peers that update by tiles).  15 steps, and 22 for the cases
   of dp_cases.LONG_CASES, which before the tail cross every replica's 16th gradient computation (runtime-shape kernels ->
   instantiated ones).  DIRECT, DIRECT_RS and DIRECT taken one gradient_step_range at a time agree bitwise;
c. the oracles on the WHOLE batch, over the steps before the short tail (12, or 19 for a long case): f32 weights and
   momentum against the fp64 C oracle within 2e-6 per step; bf16 against the
   bf16-aware numpy oracle after 3 and 5 steps within 2e-4 / 4e-4 (the bounds of tests/test_chain_shapes_gpu.py: sharding
   changes only the order of an f32 accumulation).  The tail is held by a alone: on a batch of a few rows one ReLU
   derivative that f32 takes on the other side of zero moves a weight by many budgets (measured in fp64 by
   tests/test_dp_cases_cpu.py::test_a_batch_of_a_few_rows_is_outside_the_oracle_budget).  The bf16 checkpoints are read
   from the DIRECT and the DIRECT_RS handle, which must agree bitwise there too;
d. what the f32 budget catches of a wrong data-parallel step was measured on the reference side
   (tests/test_dp_cases_cpu.py: a dropped partial gradient 26 of 26 cases, a mean of shard means 17 of 26 -- every case with
   unequal shards --, an owner's slice left unreduced 26 of 26, one narrowly; a stale slice 25 of 26); a is what holds the rest;
e. evaluation through the LAST replica: propagate and count_hits_range bitwise equal to replica 0's; f32: loss_range and
   argmax_range against the oracle at the tolerances of test_chained_loops_f32;
f. GNN_REDUCE_RCCL on a world of one (a dp handle, and gnn_mlp_rccl_train_range on a lone handle) bitwise equal to the
   one-rank reference, six cases;
g. floors on the kernels the sweep runs on, read from fresh handles.

Measured on an MI355X: every case uses at most 0.004 of the f32 budget and 0.047 of the bf16 bounds.  Five deliberate
breakages, each built on a scratch copy, fail the sweep by the bitwise checks of a (eight or more cases each): the owner in
ts_gradient_in<4> capped at n_peer - 2; `r < p.n - 1` in direct_reduce_update_kernel; the same in
direct_reduce_scatter_kernel; the memset of a replica without rows dropped in dp_step_range_body (which nothing else in the
suite notices: it needs a replica that had rows two steps earlier); the same memset dropped in gnn_mlp_dp_gradient_step."""
import numpy as np
import pytest

from tests import chain_cases as cc
from tests import dp_cases as dc
from tests import np_oracle
from tests.test_chain_shapes_gpu import W_ATOL, _forced_path

pytestmark = pytest.mark.gpu

CASES = range(dc.N_DP_CASES)
RCCL_CASES = [(7, "f32"), (7, "bf16"), (2, "f32"), (2, "bf16"), (4, "f32"), (10, "f32"), (13, "f32"), (21, "f32")]


def _dtype(gnn, dtype):
    return gnn.DTYPE_BF16 if dtype == "bf16" else gnn.DTYPE_F32


def _lone(gnn, i, dt, w0, X, Y):
    dims, B, inner, out_kind, last, _, _ = dc.dp_case(i)
    if out_kind == cc.OUT_SOFTMAX_CE:
        net = gnn.SoftmaxCrossEntropyNeuralNet(dims, inner_act=inner, dtype=dt, max_batch=B)
    else:
        net = gnn.GeneralNeuralNet(dims, inner_act=inner, last_act=last, dtype=dt, max_batch=B)
    net.set_weights(w0)
    net.upload_dataset(X, Y)
    return net


def _dp(gnn, i, dt, reducer, w0, X, Y, n=None):
    dims, B, inner, out_kind, last, n_case, _ = dc.dp_case(i)
    net = gnn.DataParallelNeuralNet(dims, devices=[0] * (n or n_case), out_kind=out_kind, inner_act=inner, last_act=last, dtype=dt,
                                    max_batch=B, reducer=reducer)
    net.set_weights(w0)                                  # (gnn_mlp_dp_set_weights: the handle's only setter; momentum starts at zero)
    net.upload_dataset(X, Y)
    return net


def _path(net):
    return net.step_launches, net.rowblock_state, net.plan_note


def _assert_bitwise(x, y, what):
    assert x.time == y.time, "time differs (%d, %d): %s" % (x.time, y.time, what)
    wx, wy = x.get_weights(), y.get_weights()
    if not np.array_equal(wx, wy):
        bad = np.flatnonzero(wx != wy)
        ends = np.cumsum([a * b for a, b in zip(x.layer_dims[:-1], x.layer_dims[1:])])
        layer = [int(np.searchsorted(ends, k, side="right")) for k in bad[:4]]
        raise AssertionError("weights differ (%s): %d of %d elements, max %.3g, first at %r in layers %r"
                             % (what, bad.size, wx.size, np.abs(wx - wy).max(), bad[:4].tolist(), layer))
    vx, vy = x.get_momentum(), y.get_momentum()
    assert np.array_equal(vx, vy), "momentum differs (%s): %d elements" % (what, int((vx != vy).sum()))


def _walk_dp(net, B, X, Y, long_case, stepwise=False, after_call=None):
    """The calls of dp_cases.walk_calls on a data-parallel handle; stepwise: every step as one gradient_step_range."""
    N = cc.dataset_rows(B)
    for k, call in enumerate(dc.walk_calls(B, len(net.replicas), long_case)):
        kind, first, rows = call[:3]
        if kind == "train" and not stepwise:
            net.train_range(first, rows, call[3], cc.STEP, cc.MOMENTUM)
        elif kind == "train":
            for r in cc.range_batches(N, rows, first, call[3]):
                net.gradient_step_range(r, rows, cc.STEP, cc.MOMENTUM)
        elif kind == "step" or stepwise:
            net.gradient_step_range(first, rows, cc.STEP, cc.MOMENTUM)
        else:
            net.gradientStep(X[first:first + rows], cc.STEP, cc.MOMENTUM, False, expected=Y[first:first + rows])
        if after_call is not None:
            after_call(k)
    net.synchronize()


class _HookReference:
    """n ranks as lone handles (created like the replicas: the same max_batch, so the same plan), stepped through
    bind_grad_buffer / [hint_next_range] / compute_gradient_range / apply_update with the sum taken by torch in rank order."""

    def __init__(self, gnn, torch, i, dt, w0, X, Y, n, hinted):
        self.torch, self.hinted, self.n = torch, hinted, n
        self.B = dc.dp_case(i)[1]
        self.N = cc.dataset_rows(self.B)
        self.ranks = [_lone(gnn, i, dt, w0, X, Y) for _ in range(n)]
        self.elems = self.ranks[0].grad_elems
        assert self.elems == dc.n_pad(dc.dp_case(i)[0])

    def _sync(self):
        for net in self.ranks:
            net.synchronize()
        self.torch.cuda.synchronize()

    def step(self, first, B, announce):
        """One global step on rows [first, first + B); announce: first row of the batch (of B rows) a rank names as its next."""
        torch, n = self.torch, self.n
        parts = [torch.zeros(self.elems, dtype=torch.float32, device="cuda") for _ in range(n)]   # a fresh zeroed buffer each
        self._sync()
        for r, net in enumerate(self.ranks):
            lo, hi = dc.shard(B, r, n)
            if hi == lo:
                continue                                  # a rank without rows contributes zeros
            net.bind_grad_buffer(parts[r].data_ptr(), self.elems)
            if self.hinted:
                net.hint_next_range(announce + lo, hi - lo)
            net.compute_gradient_range(first + lo, hi - lo)
        self._sync()
        g = parts[0].clone()
        for p in parts[1:]:
            g += p                                        # rank order, one f32 add per element and rank
        self._sync()
        for net in self.ranks:
            net.bind_grad_buffer(g.data_ptr(), self.elems)
            net.apply_update(B, cc.STEP, cc.MOMENTUM)
        self._sync()                                      # (g and the partial buffers are released when this returns)
        for net in self.ranks:
            net.bind_grad_buffer(0, 0)                    # back to the handle's own buffer

    def run(self, steps, snapshot_after=()):
        """steps: dp_cases.walk; returns {number of steps: (weights, momentum)} for the counts in snapshot_after."""
        snaps = {}
        for s, (kind, first, rows) in enumerate(steps):
            # what a caller that knows its walk announces: the next step's rows where that step has as many, else (as
            # train_range does at the end of a call) the batch that follows in the data set
            if s + 1 < len(steps) and steps[s + 1][2] == rows:
                announce = steps[s + 1][1]
            else:
                announce = ((first // rows + 1) % (self.N // rows)) * rows
            self.step(first, rows, announce)
            if s + 1 in snapshot_after:
                snaps[s + 1] = (self.ranks[0].get_weights(), self.ranks[0].get_momentum())
        for net in self.ranks[1:]:
            _assert_bitwise(net, self.ranks[0], "the ranks of the hook reference among themselves")
        return snaps

    def close(self):
        for net in self.ranks:
            net.close()


def _evaluate(net, i, X, Y, oracle_mod, dtype):
    """e: the last replica against replica 0 (bitwise) and, f32, against the oracle holding the same weights."""
    dims, B, inner, out_kind, last, n, _ = dc.dp_case(i)
    N = cc.dataset_rows(B)
    r0, rl = net.replicas[0], net.replicas[-1]
    assert np.array_equal(rl.propagate(X[:B]), r0.propagate(X[:B])), "propagate differs between replica 0 and the last"
    hits = rl.count_hits_range(0, N)
    assert hits == r0.count_hits_range(0, N)
    if dtype != "f32":
        return
    ref, _ = dc.case_oracle(oracle_mod, i)
    ref.set_weights(rl.get_weights())

    def safe_rows(Xr):                                    # rows whose two largest outputs are apart by more than f32 can blur
        z = ref.logits(Xr) if out_kind == cc.OUT_SOFTMAX_CE else ref.propagate(Xr)
        s = np.sort(z, axis=1)
        return (s[:, -1] - s[:, -2]) > (1e-3 if out_kind == cc.OUT_SOFTMAX_CE else 1e-4)
    for first, rows in ((0, B), (5 * B, N - 5 * B)):
        Xr, Yr = X[first:first + rows], Y[first:first + rows]
        lr = ref.calculate_loss(Xr, Yr)
        assert np.all(np.abs(rl.loss_range(first, rows) - lr) <= 1e-4 * np.abs(lr) + 1e-5), (dc.CASE_IDS[i], first, rows)
        safe = safe_rows(Xr)
        assert np.array_equal(rl.argmax_range(first, rows)[safe], ref.argmax(Xr)[safe]), (dc.CASE_IDS[i], first, rows)
    unsafe = int((~safe_rows(X)).sum())
    ref_hits = int((ref.argmax(X) == Y.argmax(axis=1)).sum())
    assert abs(hits - ref_hits) <= unsafe, (dc.CASE_IDS[i], hits, ref_hits, unsafe)


def _sweep(gnn, oracle_mod, i, dtype):
    import torch
    dims, B, inner, out_kind, last, n, _ = dc.dp_case(i)
    long_case = i in dc.LONG_CASES
    dt = _dtype(gnn, dtype)
    X, Y = dc.case_data(i)
    ref, w0 = dc.case_oracle(oracle_mod, i)
    steps = dc.walk(B, n, long_case)
    what = "%s %s n %d shards %r" % (dc.CASE_IDS[i], dtype, n, dc.shard_sizes(B, n))

    # the handles under test
    direct = _dp(gnn, i, dt, gnn.REDUCE_DIRECT, w0, X, Y)
    assert len(direct.replicas) == n and np.array_equal(direct.get_weights(), w0)
    path0 = _path(direct.replicas[0])
    checkpoints = {}

    n_calls = len(dc.walk_calls(B, n, long_case))
    oracle_steps = len(steps) - dc.TAIL_STEPS             # the oracle budgets apply up to the short tail (dp_cases.walk_calls)

    def after_call(k):                                    # calls 0 and 1 end after 3 and 5 steps
        if (dtype == "bf16" and k in (0, 1)) or k == n_calls - dc.TAIL_CALLS - 1:
            direct.synchronize()
            checkpoints[3 if k == 0 else 5 if k == 1 else oracle_steps] = (direct.get_weights(), direct.get_momentum())
    _walk_dp(direct, B, X, Y, long_case, after_call=after_call)
    direct_rs = _dp(gnn, i, dt, gnn.REDUCE_DIRECT_RS, w0, X, Y)
    checkpoints_rs = {}

    def after_call_rs(k):
        if dtype == "bf16" and k in (0, 1):
            direct_rs.synchronize()
            checkpoints_rs[3 if k == 0 else 5] = (direct_rs.get_weights(), direct_rs.get_momentum())
    _walk_dp(direct_rs, B, X, Y, long_case, after_call=after_call_rs)
    for k, (w_rs, v_rs) in checkpoints_rs.items():
        assert np.array_equal(w_rs, checkpoints[k][0]) and np.array_equal(v_rs, checkpoints[k][1]), "DIRECT_RS against DIRECT after %d steps, %s" % (k, what)
    stepwise = _dp(gnn, i, dt, gnn.REDUCE_DIRECT, w0, X, Y)
    _walk_dp(stepwise, B, X, Y, long_case, stepwise=True)
    stepwise_rs = _dp(gnn, i, dt, gnn.REDUCE_DIRECT_RS, w0, X, Y)
    _walk_dp(stepwise_rs, B, X, Y, long_case, stepwise=True)
    path1 = _path(direct.replicas[0])

    # a: the reference from the one-GPU hooks, plain and announced
    plain = _HookReference(gnn, torch, i, dt, w0, X, Y, n, hinted=False)
    plain.run(steps)
    hinted = _HookReference(gnn, torch, i, dt, w0, X, Y, n, hinted=True)
    hinted.run(steps)

    # c: the oracles on the whole batch
    if dtype == "f32":
        for _, first, rows in steps[:oracle_steps]:
            ref.gradient_step(X[first:first + rows], Y[first:first + rows], cc.STEP, cc.MOMENTUM)
        budget = W_ATOL * oracle_steps
        dw = np.abs(checkpoints[oracle_steps][0] - ref.get_weights()).max()
        dv = np.abs(checkpoints[oracle_steps][1] - ref.get_momentum()).max()
        used = "dw %.3f dv %.3f of the budget (%d steps)" % (dw / budget, dv / budget, oracle_steps)
    else:
        X32 = X.astype(np.float32).astype(np.float64)     # inputs are f32 in HBM
        w, v = w0.copy(), np.zeros_like(w0)
        dev = {}
        for s, (_, first, _) in enumerate(steps[:5]):
            w, v = np_oracle.gradient_step_bf16(w, v, dims, X32[first:first + B], Y[first:first + B], cc.STEP, cc.MOMENTUM, inner, out_kind, last)
            if s + 1 in (3, 5):
                dev[s + 1] = (np.abs(checkpoints[s + 1][0] - w).max(), np.abs(checkpoints[s + 1][1] - v).max())
        used = "after 3 steps dw %.3f dv %.3f of 2e-4, after 5 dw %.3f dv %.3f of 4e-4" % (dev[3][0] / 2e-4, dev[3][1] / 2e-4, dev[5][0] / 4e-4, dev[5][1] / 4e-4)
    print("dp-case %s %s dims %s B %d act %d out %d/%d | replicas %d shards %s | launches %d rowblock %d->%d note %r | %s"
          % (dc.CASE_IDS[i], dtype, "-".join(map(str, dims)), B, inner, out_kind, last, n, ",".join(map(str, dc.shard_sizes(B, n))),
             path0[0], path0[1], path1[1], path0[2], used))

    assert direct.time == len(steps)
    for net, name in ((direct, "DIRECT"), (direct_rs, "DIRECT_RS"), (stepwise, "DIRECT stepwise"), (stepwise_rs, "DIRECT_RS stepwise")):
        assert net.replicas_identical(), "replicas differ: %s, %s" % (name, what)
        _assert_bitwise(net, plain.ranks[0], "%s against the hook reference, %s, %r" % (name, what, path1))
        _assert_bitwise(net, hinted.ranks[0], "%s against the announced hook reference, %s, %r" % (name, what, path1))
        _assert_bitwise(net, direct, "%s against DIRECT, %s" % (name, what))
    if dtype == "f32":
        assert dw <= budget and dv <= budget, (what, path1, dw, dv)
    else:
        assert dev[3][0] <= 2e-4 and dev[3][1] <= 2e-4, (what, path1, dev)
        assert dev[5][0] <= 4e-4 and dev[5][1] <= 4e-4, (what, path1, dev)

    # e: evaluation through the last replica
    _evaluate(direct_rs, i, X, Y, oracle_mod, dtype)
    _evaluate(direct, i, X, Y, oracle_mod, dtype)
    for net in (direct, direct_rs, stepwise, stepwise_rs, plain, hinted):
        net.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("i", [i for i in CASES if dc.dp_case(i)[5] < 16], ids=lambda i: dc.CASE_IDS[i])
def test_dp_sweep(gnn, oracle_mod, i, dtype):
    if _forced_path():
        pytest.skip("path forced by the environment")
    _sweep(gnn, oracle_mod, i, dtype)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("i", [i for i in CASES if dc.dp_case(i)[5] == 16], ids=lambda i: dc.CASE_IDS[i])
def test_dp_sweep_sixteen_replicas(gnn, oracle_mod, i, dtype):
    """DP_MAX_REPLICAS replicas on one device.  x2 gives every replica rows, so the `if (r < p.n)` chains of the reducers run
    full with a real partial gradient in every term, the 16th included; in the other cases most replicas have no rows (a
    memset for a gradient, no announcement, the flat update next to peers that update by tiles)."""
    if _forced_path():
        pytest.skip("path forced by the environment")
    _sweep(gnn, oracle_mod, i, dtype)


@pytest.mark.parametrize("i,dtype", RCCL_CASES, ids=lambda p: dc.CASE_IDS[p] if isinstance(p, int) else p)
def test_rccl_world_of_one(gnn, oracle_mod, i, dtype):
    """f: GNN_REDUCE_RCCL with one replica takes the whole walk; a lone handle with a communicator of one rank takes the
    train_range calls through gnn_mlp_rccl_train_range.  Both equal the one-rank hook reference bit for bit."""
    import torch
    if _forced_path():
        pytest.skip("path forced by the environment")
    dims, B, inner, out_kind, last, _, _ = dc.dp_case(i)
    dt = _dtype(gnn, dtype)
    X, Y = dc.case_data(i)
    _, w0 = dc.case_oracle(oracle_mod, i)
    steps = dc.walk(B, 1)
    n_range = sum(n for _, n in dc.RANGE_CALLS)
    assert [(k, rows) for k, _, rows in steps[:n_range]] == [("range", B)] * n_range
    plain = _HookReference(gnn, torch, i, dt, w0, X, Y, 1, hinted=False)
    snaps = plain.run(steps, snapshot_after=(n_range,))

    net = _dp(gnn, i, dt, gnn.REDUCE_RCCL, w0, X, Y, n=1)
    _walk_dp(net, B, X, Y, False)
    assert net.replicas_identical()
    _assert_bitwise(net, plain.ranks[0], "RCCL dp handle against the hook reference, %s %s" % (dc.CASE_IDS[i], dtype))

    lone = _lone(gnn, i, dt, w0, X, Y)
    lone.rccl_attach(gnn.NeuralNet.rccl_unique_id(), 1, 0)
    for first, n in dc.RANGE_CALLS:
        lone.rccl_train_range(first * B, B, n, cc.STEP, cc.MOMENTUM)
    lone.synchronize()
    assert lone.time == n_range
    assert np.array_equal(lone.get_weights(), snaps[n_range][0]) and np.array_equal(lone.get_momentum(), snaps[n_range][1]), \
        "rccl_train_range against the hook reference, %s %s %r" % (dc.CASE_IDS[i], dtype, _path(lone))
    lone.rccl_detach()
    for x in (net, lone, plain):
        x.close()


def test_the_dp_sweep_runs_on_the_kernels_it_is_for(gnn):
    """g: conditions on the cases, read from fresh handles.  f32, multi-replica: at least 12 cases whose replicas take the
    two-launch step (train_range then runs the fused GSRC = 3 / 4 tile kernel) and at least 3 that do not (the flat kernels
    alone); bf16, multi-replica, two-launch: both row kernels occur."""
    if _forced_path():
        pytest.skip("path forced by the environment")
    paths = {}
    for dtype in ("f32", "bf16"):
        for i in CASES:
            dims, B, inner, out_kind, last, n, _ = dc.dp_case(i)
            if n == 1:
                continue
            net = gnn.DataParallelNeuralNet(dims, devices=[0, 0], out_kind=out_kind, inner_act=inner, last_act=last,
                                            dtype=_dtype(gnn, dtype), max_batch=B, reducer=gnn.REDUCE_DIRECT)
            paths[dtype, i] = _path(net.replicas[1])
            assert paths[dtype, i] == _path(net.replicas[0])
            net.close()
    f32 = [p for (d, _), p in paths.items() if d == "f32"]
    bf16 = [p for (d, _), p in paths.items() if d == "bf16"]
    assert sum(1 for p in f32 if p[0] == 2) >= 12, f32
    assert sum(1 for p in f32 if p[0] != 2) >= 3, f32
    assert any(p[0] == 0 for p in f32), f32                                   # (the per-layer GEMM form: the two-layer extra)
    assert any(p[0] == 2 and p[1] != 0 for p in bf16) and any(p[0] == 2 and p[1] == 0 for p in bf16), bf16
