"""NetGroup.evaluate_range / ensemble_propagate_range / ensemble_argmax_range (gnn_mlp_group_evaluate_range, _ensemble_range):
every member's hits and loss sum and the ensemble's mean output over rows of the group's data set, in grouped launches
(csrc/group_eval_kernel.h) or, where the kernel does not apply (E7, E7b, E7g), member after member.

Against the fp64 oracle, labels and hits are compared on rows whose top-2 margin exceeds the project's budgets
(tests/group_eval_cases.py; tests/test_group_eval_cpu.py pins how few rows fall below them); outputs to the probability
budgets of test_parity_gpu.py (2e-4, f32) and test_bf16_gpu.py (5e-3, bf16)."""
import numpy as np
import pytest

from tests import group_eval_cases as gc

pytestmark = pytest.mark.gpu


def _group(gnn, case, weights, Y, K=None, max_batch=1024):
    K = case.K if K is None else K
    g = gnn.NetGroup(case.dims, list(range(1, K + 1)), out_kind=case.kind, inner_act=case.inner, last_act=case.last,
                     dtype=case.dtype, max_batch=max_batch)
    for k in range(K):
        g.members[k].set_weights(weights[k])
    g.upload_dataset(gc.inputs(case), Y)
    return g


def _case_group(gnn, oracle_mod, name, **kw):
    case, t = gc.CASES[name], gc.truth(oracle_mod, name)
    w = [gc.member_weights(oracle_mod, case, k) for k in range(kw.get("K") or case.K)]
    return case, t, _group(gnn, case, w, t.Y, **kw)


def _check_against(g, case, t, K):
    """The rules of the issue's test 1 for the group g against the oracle's verdict t (its first K members)."""
    n = case.rows
    mean_t = t.out[:K].mean(axis=0)
    hits, loss, ens_hits = g.evaluate_range(0, n)
    mean = g.ensemble_propagate_range(0, n)
    lab = g.ensemble_argmax_range(0, n)
    bf = case.dtype == gc.BF16
    err = np.abs(mean - mean_t).max()
    print(case.name, "K", K, "mean-output error", err, "hits", hits.tolist(), "ensemble hits", ens_hits)
    assert err <= (5e-3 if bf else 2e-4)
    if K == t.out.shape[0]:
        ens_label, ens_safe = t.ens_label, t.ens_safe
    else:  # (fewer members than the fixture: the same dtype rule on THIS group's mean output)
        srt = np.sort(mean_t, axis=1)
        ens_safe = (srt[:, -1] - srt[:, -2]) > (2e-3 * np.abs(mean_t).max() + 1e-3 if bf else 1e-3)
        ens_label = np.array([int(np.flatnonzero(r >= r.max())[-1]) for r in mean_t])  # `>=`: ties to the highest index
    assert np.array_equal(lab[ens_safe], ens_label[ens_safe])
    lo, hi = t.hits_bounds(ens_label, ens_safe)
    assert lo <= ens_hits <= hi
    for k in range(K):
        lo, hi = t.hits_bounds(t.label[k], t.safe[k])
        assert lo <= hits[k] <= hi, "member %d" % k
        unsafe = int((~t.safe[k]).sum())
        assert abs(int(hits[k]) - g.members[k].count_hits_range(0, n)) <= unsafe, "member %d" % k
        own = g.members[k].loss_range(0, n)
        d_own = abs(loss[k] - own.sum())
        d_ref = abs(loss[k] - t.loss[k].sum())
        print("  member", k, "loss sum", loss[k], "own", own.sum(), "oracle", t.loss[k].sum())
        assert d_own <= (1e-4 * np.abs(own) + 1e-5).sum(), "member %d" % k
        if not bf:
            assert d_ref <= (2e-4 * np.abs(t.loss[k]) + 2e-4).sum(), "member %d" % k


@pytest.mark.parametrize("name", gc.NAMES)
def test_against_fp64_oracle(gnn, oracle_mod, name):
    case, t, g = _case_group(gnn, oracle_mod, name)
    assert g.eval_launches == (2 if case.grouped else 0)
    for k in range(case.K):  # the oracle's members hold the group's weights
        assert np.array_equal(g.members[k].get_weights(), gc.member_weights(oracle_mod, case, k))
    _check_against(g, case, t, case.K)
    g.close()


@pytest.mark.parametrize("name", ["E1", "E1b"])
def test_single_member_group(gnn, oracle_mod, name):
    case, t, g = _case_group(gnn, oracle_mod, name, K=1)
    assert g.eval_launches == 2
    mean = g.ensemble_propagate_range(0, case.rows)
    assert np.array_equal(mean, mean.astype(np.float32).astype(np.float64))  # the member's own f32 output
    _check_against(g, case, t, 1)
    g.close()


@pytest.mark.parametrize("name", ["E1", "E2", "E3b", "E9b", "E10"])
def test_rows_do_not_depend_on_their_place(gnn, oracle_mod, name, monkeypatch):
    case, t, g = _case_group(gnn, oracle_mod, name)
    n = case.rows
    mean, lab = g.ensemble_propagate_range(0, n), g.ensemble_argmax_range(0, n)
    hits, loss, ens = g.evaluate_range(0, n)
    # rows [3, n - 4) on their own: other tiles, the same bits
    assert np.array_equal(g.ensemble_propagate_range(3, n - 7), mean[3:n - 4])
    assert np.array_equal(g.ensemble_argmax_range(3, n - 7), lab[3:n - 4])
    # the same call twice: the same bits in the loss sums
    hits2, loss2, ens2 = g.evaluate_range(0, n)
    assert np.array_equal(loss, loss2) and np.array_equal(hits, hits2) and ens == ens2
    # blocks of 32 rows instead of one block
    monkeypatch.setenv("GNN_MLP_EVAL_ROWS", "0")
    w = [gc.member_weights(oracle_mod, case, k) for k in range(case.K)]
    gb = _group(gnn, case, w, t.Y, max_batch=32)
    monkeypatch.delenv("GNN_MLP_EVAL_ROWS")
    assert gb.eval_launches == 2
    assert np.array_equal(gb.ensemble_propagate_range(0, n), mean)
    assert np.array_equal(gb.ensemble_argmax_range(0, n), lab)
    hb, lb, eb = gb.evaluate_range(0, n)
    assert np.array_equal(hb, hits) and eb == ens
    g.close()
    gb.close()


@pytest.mark.parametrize("name", ["E1", "E1b"])
def test_evaluation_is_invisible_to_training(gnn, oracle_mod, name):
    case, t = gc.CASES[name], gc.truth(oracle_mod, name)
    w = [gc.member_weights(oracle_mod, case, k) for k in range(case.K)]
    n, B = case.rows, 64
    steps = [0.01 + 0.002 * k for k in range(case.K)]
    moms = [0.9 - 0.02 * k for k in range(case.K)]
    groups, samplers = [], []
    for evaluate in (True, False):
        g = _group(gnn, case, w, t.Y, max_batch=B)
        s = gnn.Sampler(n, seed=1)
        g.train_range(0, B, 5, steps, moms)
        if evaluate:
            g.evaluate_range(0, n)
            g.ensemble_propagate_range(0, n)
        g.train_sampled(s, 6, B, steps, moms)
        groups.append(g)
        samplers.append(s)
    for k in range(case.K):
        a, b = groups[0].members[k], groups[1].members[k]
        assert np.array_equal(a.get_weights(), b.get_weights()), "weights of member %d" % k
        assert np.array_equal(a.get_momentum(), b.get_momentum()), "momentum of member %d" % k
        assert a.time == b.time == 11
    assert np.array_equal(samplers[0].sample(B), samplers[1].sample(B))
    for g in groups:
        g.close()
    for s in samplers:
        s.close()


def test_deferred_update_is_applied_first(gnn, oracle_mod):
    case, t, g = _case_group(gnn, oracle_mod, "E1")
    X = gc.inputs(case)
    g.members[0].gradientStep(X[:32], 0.05, 0.9, False, expected=t.Y[:32])  # a host batch: its update is pending
    hits, loss, ens_hits = g.evaluate_range(0, case.rows)
    after = gc.Truth(oracle_mod, case, [m.get_weights() for m in g.members], Y=t.Y)
    assert not np.array_equal(after.out[0], t.out[0])
    hits2, loss2, ens2 = g.evaluate_range(0, case.rows)
    assert np.array_equal(hits, hits2) and np.array_equal(loss, loss2) and ens_hits == ens2
    _check_against(g, case, after, case.K)
    g.close()


def test_refusals(gnn, oracle_mod):
    import ctypes as C
    case, t = gc.CASES["E2"], gc.truth(oracle_mod, "E2")
    w = [gc.member_weights(oracle_mod, case, k) for k in range(case.K)]
    g = gnn.NetGroup(case.dims, list(range(1, case.K + 1)), inner_act=case.inner)
    with pytest.raises(gnn.GnnError) as e:  # no data set
        g.evaluate_range(0, 4)
    assert e.value.code == 5
    with pytest.raises(gnn.GnnError) as e:
        g.ensemble_argmax_range(0, 4)
    assert e.value.code == 5
    g.close()
    g = _group(gnn, case, w, t.Y)
    n = case.rows
    before = [m.count_hits_range(0, n) for m in g.members]
    lib = g._lib
    assert lib.gnn_mlp_group_evaluate_range(None, 0, 4, None, None, C.byref(C.c_int64())) == 1   # null group
    assert lib.gnn_mlp_group_ensemble_range(None, 0, 4, None, (C.c_int32 * 4)()) == 1
    assert lib.gnn_mlp_group_evaluate_range(g._h, 0, 4, None, None, None) == 1                  # every output null
    assert lib.gnn_mlp_group_ensemble_range(g._h, 0, 4, None, None) == 1
    for first, cnt in ((0, 0), (0, -3), (-1, 4), (n - 3, 4), (n, 1), (0, n + 1)):                # rows outside the data set
        with pytest.raises(gnn.GnnError) as e:
            g.evaluate_range(first, cnt)
        assert e.value.code == 1
        with pytest.raises(gnn.GnnError) as e:
            g.ensemble_propagate_range(first, cnt)
        assert e.value.code == 1
    # single outputs are enough, and n=None means the rest of the data set
    ens = C.c_int64()
    assert lib.gnn_mlp_group_evaluate_range(g._h, 0, n, None, None, C.byref(ens)) == 0
    hits, loss, ens_hits = g.evaluate_range()
    assert ens.value == ens_hits
    hits_tail, _, _ = g.evaluate_range(n - 5)
    assert (hits_tail <= 5).all()
    # the members still work through their own handles
    assert [m.count_hits_range(0, n) for m in g.members] == before
    g.close()
