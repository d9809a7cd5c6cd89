"""The merged tile map's workgroup kinds (csrc/tile_step_body.inc: a group of layer 0's partial last tile row, a pair of a later
layer) on the cases of tests/tile_merge_cases.py: planted and drawn shapes, every batch size class, train_range walks that wrap
and end at the data set's last row, train_sampled with a shortened batch, announced steps whose padded sizes change across 128.

Per case three nets: the default one, its twin created under GNN_MLP_TILE_MERGE=0 (one tile per workgroup), the fp64 oracle.
1. which launch runs: two launches per step, the row-block kernel on the path, the twin on the one-tile map, the default on the
   merged map in exactly the grid the host checker (tests/native/tile_merge_check.hip) derives for this device's CU count -- or
   on the one-tile map where the checker says the merged one is not usable (800-300-100-10);
2. bitwise, after EVERY call of the schedule: weights, momentum and time, default against twin (merging changes who computes a
   tile and not one operation of its sums);
3. the schedule's second cut (the same steps in other calls) ends bitwise where the first did;
4. at the end weights and momentum within W_ATOL = 2e-6 per step of the oracle (tests/test_tile_merge_cases_cpu.py: the
   reference restated in float32 stays within a quarter of that, and a missing update or a stale slab piece cannot hide)."""
import os

import numpy as np
import pytest

from tests import tile_merge_cases as tc

pytestmark = pytest.mark.gpu


def _forced_path():
    e = os.environ
    return bool(e.get("GNN_MLP_PATH") or e.get("GNN_MLP_CHAIN") == "0" or e.get("GNN_MLP_ROWBLOCK") == "0" or e.get("GNN_MLP_TILE_HEAD")
                or e.get("GNN_MLP_TILE_MERGE"))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    out = tc.build_checker(tmp_path_factory.mktemp("tile_merge_cases_gpu"))
    assert out is not None, "hipcc is needed for the host checker"
    return out


@pytest.fixture(scope="module")
def cus_per_xcd():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count // 8


def _make(gnn, case, dtype=None):
    dtype = gnn.DTYPE_F32 if dtype is None else dtype
    if case.out_kind == tc.OUT_SOFTMAX_CE:
        return gnn.SoftmaxCrossEntropyNeuralNet(case.dims, inner_act=case.inner, dtype=dtype, max_batch=case.max_batch)
    return gnn.GeneralNeuralNet(case.dims, inner_act=case.inner, last_act=case.last, dtype=dtype, max_batch=case.max_batch)


class Runner:
    """A handle with the case's start weights, data set and sampler; run(call) makes one call of a schedule."""

    def __init__(self, gnn, case, w0, X, Y):
        self.net = _make(gnn, case)
        self.net.set_weights(w0)
        self.net.upload_dataset(X, Y)
        self.sampler = gnn.Sampler(case.rows, seed=tc.SAMPLER_SEED) if case.kind.startswith("sampled") else None

    def run(self, call):
        net = self.net
        if call[0] == "range":
            net.train_range(call[1], call[2], call[3], tc.STEP, tc.MOMENTUM)
        elif call[0] == "sampled":
            rc = net._lib.gnn_mlp_train_sampled(net._h, self.sampler._h, call[1], call[2], tc.STEP, tc.MOMENTUM, 0)
            assert rc == 0, rc
        else:
            if call[3] is not None:
                net.hint_next_range(*call[3])
            net.gradient_step_range(call[1], call[2], tc.STEP, tc.MOMENTUM)

    def close(self):
        self.net.close()
        if self.sampler is not None:
            self.sampler.close()


def _assert_bitwise(x, y, what):
    assert x.time == y.time, "time differs: " + what
    wx, wy = x.get_weights(), y.get_weights()
    if not np.array_equal(wx, wy):
        bad = np.flatnonzero(wx != wy)
        ends = np.cumsum([a * b for a, b in zip(x.layer_dims[:-1], x.layer_dims[1:])])
        where = [(int(l), int((i - (ends[l - 1] if l else 0)) // x.layer_dims[l + 1]), int((i - (ends[l - 1] if l else 0)) % x.layer_dims[l + 1]))
                 for i in bad[:6] for l in [int(np.searchsorted(ends, i, side="right"))]]
        raise AssertionError("weights differ (%s): %d elements, max %.3g, first at (layer, row, column) %r" % (what, bad.size, np.abs(wx - wy).max(), where))
    assert np.array_equal(x.get_momentum(), y.get_momentum()), "momentum differs: " + what


@pytest.mark.parametrize("case", tc.CASES, ids=tc.IDS)
def test_merged_kinds_against_the_one_tile_twin_and_the_oracle(gnn, oracle_mod, monkeypatch, checker, cus_per_xcd, case):
    if _forced_path():
        pytest.skip("path forced by the environment")
    X, Y = tc.case_data(case)
    _, w0 = tc.oracle_net(oracle_mod, case)
    new = Runner(gnn, case, w0, X, Y)
    cut = Runner(gnn, case, w0, X, Y) if case.recut is not None else None
    monkeypatch.setenv("GNN_MLP_TILE_MERGE", "0")           # (read once at create)
    old = Runner(gnn, case, w0, X, Y)
    monkeypatch.delenv("GNN_MLP_TILE_MERGE")

    # 1. which launch runs
    _, summary = tc.entries(checker, case.dims, cus_per_xcd)
    path = (new.net.step_launches, new.net.rowblock_state, new.net.tile_merge_state, new.net.plan_note)
    assert new.net.step_launches == 2 and old.net.step_launches == 2, path
    assert new.net.rowblock_state != 0 and old.net.rowblock_state != 0, path
    assert old.net.tile_merge_state == 0
    assert new.net.tile_merge_state == (summary["grid"] if summary["usable"] else 0), (path, summary)
    if cus_per_xcd == 32:
        assert (new.net.tile_merge_state > 0) == (case.dims != tc.NOT_USABLE), path
    assert np.array_equal(new.net.get_weights(), w0)

    # 2. bitwise after every call
    for n, call in enumerate(case.schedule):
        new.run(call)
        old.run(call)
        _assert_bitwise(new.net, old.net, "after call %d %r, %r" % (n, call[:3], path))
    steps = tc.n_steps(case.schedule)
    assert new.net.time == steps
    assert new.net.rowblock_state == path[1]                # (no run-time instantiation inside the schedule)

    # 3. the same steps cut into other calls
    if cut is not None:
        for call in case.recut:
            cut.run(call)
        _assert_bitwise(cut.net, new.net, "the second cut, %r" % (path,))
        if cut.sampler is not None:
            assert np.array_equal(cut.sampler.sample(7), new.sampler.sample(7)), "the cuts left the samplers at different places"

    # 4. the oracle
    _, w, v = tc.trajectory(oracle_mod, case)
    budget = tc.W_ATOL * steps
    dw, dv = np.abs(new.net.get_weights() - w).max(), np.abs(new.net.get_momentum() - v).max()
    print("tile-merge case %s act %d out %d/%d | launches %d rowblock %d merged grid %d | dw %.3f dv %.3f of the budget %.3g"
          % (case.name, case.inner, case.out_kind, case.last, path[0], path[1], path[2], dw / budget, dv / budget, budget))
    assert dw <= budget and dv <= budget, (case.name, path, dw, dv, budget)
    for r in (new, old, cut):
        if r is not None:
            r.close()


def test_bf16_net_of_a_usable_shape_keeps_the_one_tile_map(gnn):
    """The merged kinds exist in the f32 kernel only: a bf16 net of a shape whose f32 form runs them reports the one-tile map."""
    if _forced_path():
        pytest.skip("path forced by the environment")
    case = next(c for c in tc.CASES if c.dims == [65, 100, 70, 10] and c.out_kind == tc.OUT_SOFTMAX_CE)
    f32, bf16 = _make(gnn, case), _make(gnn, case, gnn.DTYPE_BF16)
    assert f32.step_launches == 2 and f32.tile_merge_state > 0
    assert bf16.step_launches == 2 and bf16.tile_merge_state == 0
    f32.close(); bf16.close()
