"""Confusion matrices in one pass (gnn_mlp_evaluate_range, gnn_mlp_group_confusion_range; csrc/confusion_kernel.h): a lone net's,
every group member's and the ensemble's, counted on the device from the labels of an evaluation pass.

The counts are integer: every comparison with a numpy count of the returned labels is EXACT.  Against the fp64 oracle the
labels are compared on the rows tests/group_eval_cases.py marks safe; tests/test_confusion_cpu.py pins that the fixtures'
matrices are far from symmetric (a swapped row / column convention cannot pass) and that several classes are predicted."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import group_eval_cases as gc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def count(expected, labels, d):
    m = np.zeros((d, d), dtype=np.int64)
    np.add.at(m, (np.asarray(expected), np.asarray(labels)), 1)
    return m


def expected_rule(Y):
    """MT:186-188: the LAST index whose expected value is exactly 1, 0 when there is none."""
    return np.array([int(np.flatnonzero(r == 1.0)[-1]) if (r == 1.0).any() else 0 for r in np.asarray(Y)], dtype=np.int64)


def _group(gnn, case, weights, Y, max_batch=1024):
    g = gnn.NetGroup(case.dims, list(range(1, case.K + 1)), out_kind=case.kind, inner_act=case.inner, last_act=case.last,
                     dtype=case.dtype, max_batch=max_batch)
    for k in range(case.K):
        g.members[k].set_weights(weights[k])
    g.upload_dataset(gc.inputs(case), Y)
    return g


def _weights(oracle_mod, case):
    return [gc.member_weights(oracle_mod, case, k) for k in range(case.K)]


def _case_group(gnn, oracle_mod, name, **kw):
    case, t = gc.CASES[name], gc.truth(oracle_mod, name)
    return case, t, _group(gnn, case, _weights(oracle_mod, case), t.Y, **kw)


# ---- 1. groups ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["E2", "E3", "E4", "E6c", "E1b", "E7", "E7g"])
def test_group_matrices_are_the_counts_of_the_labels(gnn, oracle_mod, name):
    case, t, g = _case_group(gnn, oracle_mod, name)
    assert g.eval_launches == (2 if case.grouped else 0)
    n, d, K = case.rows, case.dims[-1], case.K
    member, ens, lab = g.confusion_range(0, n, labels=True)
    assert member.shape == (K, d, d) and ens.shape == (d, d) and lab.shape == (K, n)
    assert member.dtype == np.int64 and ens.dtype == np.int64 and lab.dtype == np.int32
    hits, loss, ens_hits = g.evaluate_range(0, n)
    ens_lab = g.ensemble_argmax_range(0, n)
    rows_per_class = np.bincount(t.expected, minlength=d)
    print(name, "hits", hits.tolist(), "ensemble hits", ens_hits, "off-diagonal (ensemble)", int(ens.sum() - np.trace(ens)))
    for k in range(K):
        assert np.array_equal(member[k], count(t.expected, lab[k], d)), "member %d" % k
        assert np.trace(member[k]) == hits[k], "member %d" % k
        assert member[k].sum() == n and np.array_equal(member[k].sum(axis=1), rows_per_class), "member %d" % k
        assert np.array_equal(lab[k][t.safe[k]], t.label[k][t.safe[k]]), "member %d" % k
    assert np.array_equal(ens, count(t.expected, ens_lab, d))
    assert np.trace(ens) == ens_hits
    assert ens.sum() == n and np.array_equal(ens.sum(axis=1), rows_per_class)
    # single outputs are enough, and without labels the same matrices
    member2, ens2 = g.confusion_range(0, n)
    assert np.array_equal(member2, member) and np.array_equal(ens2, ens)
    only = np.zeros((d, d), dtype=np.int64)
    assert g._lib.gnn_mlp_group_confusion_range(g._h, 0, n, None, only.ctypes.data_as(C.POINTER(C.c_int64)), None) == 0
    assert np.array_equal(only, ens)
    g.close()


# ---- 2. place and blocks -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["E2", "E1b", "E7g"])
def test_matrices_do_not_depend_on_place_or_blocks(gnn, oracle_mod, name, monkeypatch):
    case, t, g = _case_group(gnn, oracle_mod, name)
    n, d, K = case.rows, case.dims[-1], case.K
    member, ens, lab = g.confusion_range(0, n, labels=True)
    ens_lab = g.ensemble_argmax_range(0, n)
    # rows [3, n - 4) on their own: the counts of that slice of the labels
    ms, es, ls = g.confusion_range(3, n - 7, labels=True)
    assert np.array_equal(ls, lab[:, 3:n - 4])
    for k in range(K):
        assert np.array_equal(ms[k], count(t.expected[3:n - 4], lab[k, 3:n - 4], d)), "member %d" % k
    assert np.array_equal(es, count(t.expected[3:n - 4], ens_lab[3:n - 4], d))
    # the same call twice: the same arrays
    m2, e2, l2 = g.confusion_range(0, n, labels=True)
    assert np.array_equal(m2, member) and np.array_equal(e2, ens) and np.array_equal(l2, lab)
    # blocks of 32 rows instead of one block
    monkeypatch.setenv("GNN_MLP_EVAL_ROWS", "0")
    gb = _group(gnn, case, _weights(oracle_mod, case), t.Y, max_batch=32)
    monkeypatch.delenv("GNN_MLP_EVAL_ROWS")
    assert gb.eval_launches == (2 if case.grouped else 0)
    mb, eb, lb = gb.confusion_range(0, n, labels=True)
    assert np.array_equal(lb, lab)
    assert np.array_equal(mb, member) and np.array_equal(eb, ens)
    g.close()
    gb.close()


# ---- 3. lone handles ---------------------------------------------------------------------------------------------------------
def _check_lone(net, t, k, n, d):
    """net holds the weights of the fixture's member k and the fixture's data set."""
    hits, loss_sum = net.evaluate_range(0, n)
    assert hits == net.count_hits_range(0, n)
    own = net.loss_range(0, n)
    print("  loss sum", loss_sum, "sum of loss_range", own.sum(), "hits", hits)
    assert abs(loss_sum - own.sum()) <= (1e-4 * np.abs(own) + 1e-5).sum()
    lab = net.labels_range(0, n)
    assert lab.dtype == np.int32 and lab.shape == (n,)
    conf = net.confusion_range(0, n)
    assert np.array_equal(conf, count(t.expected, lab, d))
    assert np.trace(conf) == hits and conf.sum() == n
    assert np.array_equal(lab, net.argmax_range(0, n))  # n <= max_batch: the same path
    assert np.array_equal(lab[t.safe[k]], t.label[k][t.safe[k]])
    # a range that starts inside the data set, and n=None = the rest of it
    part = net.labels_range(5, n - 9)
    assert np.array_equal(net.confusion_range(5, n - 9), count(t.expected[5:n - 4], part, d))
    assert np.array_equal(part[t.safe[k][5:n - 4]], t.label[k][5:n - 4][t.safe[k][5:n - 4]])
    tail = net.labels_range(n - 11)
    assert tail.shape == (11,) and np.array_equal(net.confusion_range(n - 11), count(t.expected[n - 11:], tail, d))
    assert net.evaluate_range() == (hits, loss_sum)


@pytest.mark.parametrize("name", ["E2", "E6c", "E7g"])   # 65-33-17-10 f32, 300-120-12 bf16, General 120-50-20
def test_lone_handle(gnn, oracle_mod, name):
    case, t = gc.CASES[name], gc.truth(oracle_mod, name)
    n, d = case.rows, case.dims[-1]
    net = gnn.NeuralNet(case.dims, case.kind, case.inner, case.last, gnn.LOSS_HALF_SQUARED, dtype=case.dtype)
    net.set_weights(gc.member_weights(oracle_mod, case, 0))
    net.upload_dataset(gc.inputs(case), t.Y)
    _check_lone(net, t, 0, n, d)
    net.close()
    # the same on a borrowed handle: member 1 of a group
    g = _group(gnn, case, _weights(oracle_mod, case), t.Y)
    _check_lone(g.members[1], t, 1, n, d)
    g.close()


# ---- 4. row counts and the expected-class rule -------------------------------------------------------------------------------
def _chunk_rows():
    text = open(os.path.join(ROOT, "graph-neural-net_amd", "csrc", "confusion_kernel.h")).read()
    return int(re.search(r"constexpr int CF_CHUNK = (\d+);", text).group(1))


def test_row_counts_and_expected_class_rule(gnn):
    chunk = _chunk_rows()
    N, d = chunk + 1, 10
    rng = np.random.default_rng(77)
    X = rng.standard_normal((N, 20))
    cls = rng.integers(0, d, N)
    Y = np.eye(d)[cls]
    Y[0] = 0.0                                        # no 1 at all: class 0
    Y[1] = 0.0; Y[1, 2] = 1.0; Y[1, 7] = 1.0          # two ones: the last
    Y[2] = 0.5                                        # no value is exactly 1: class 0
    Y[N - 1] = 0.0; Y[N - 1, 3] = 1.0; Y[N - 1, 9] = 1.0
    Y[40] = 0.0; Y[41] = 0.5; Y[300] = 0.0; Y[300, 0] = 1.0; Y[300, 4] = 1.0
    expected = expected_rule(Y)
    assert expected[0] == 0 and expected[1] == 7 and expected[2] == 0 and expected[N - 1] == 9 and expected[300] == 4
    net = gnn.GeneralNeuralNet([20, 12, d], inner_act=gnn.ACT_IDENTITY, last_act=gnn.ACT_SIGMOID)
    net.upload_dataset(X, Y)
    for n in (1, 63, 257, N):
        lab = net.labels_range(0, n)
        conf = net.confusion_range(0, n)
        hits, _ = net.evaluate_range(0, n)
        assert len(set(lab.tolist())) >= (1 if n == 1 else 3)
        assert np.array_equal(conf, count(expected[:n], lab, d)), "n = %d" % n
        assert hits == int((lab == expected[:n]).sum()) == net.count_hits_range(0, n), "n = %d" % n
    # the last rows, a range that starts inside the data set
    lab = net.labels_range(N - 63, 63)
    assert np.array_equal(net.confusion_range(N - 63, 63), count(expected[N - 63:], lab, d))
    net.close()


# ---- 5. the NaN rule ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["E2", "E7"])
def test_nan_member_predicts_class_0(gnn, oracle_mod, name):
    """A9: any NaN logit makes every probability NaN, and the `>=` argmax of a row of NaNs is 0."""
    case, t, g = _case_group(gnn, oracle_mod, name)
    n, d = case.rows, case.dims[-1]
    member, ens, lab = g.confusion_range(0, n, labels=True)
    g.members[1].set_weights(np.full(g.members[1].n_params, np.nan))
    member2, ens2, lab2 = g.confusion_range(0, n, labels=True)
    assert (lab2[1] == 0).all()
    want = np.zeros((d, d), dtype=np.int64)
    want[:, 0] = np.bincount(t.expected, minlength=d)
    assert np.array_equal(member2[1], want)
    for k in range(case.K):
        if k != 1:
            assert np.array_equal(member2[k], member[k]) and np.array_equal(lab2[k], lab[k]), "member %d" % k
    g.close()


# ---- 6. invisible to training ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["E1", "E1b"])
def test_confusion_is_invisible_to_training(gnn, oracle_mod, name):
    case, t = gc.CASES[name], gc.truth(oracle_mod, name)
    w = _weights(oracle_mod, case)
    n, B = case.rows, 64
    steps = [0.01 + 0.002 * k for k in range(case.K)]
    moms = [0.9 - 0.02 * k for k in range(case.K)]
    groups, samplers = [], []
    for evaluate in (True, False):
        g = _group(gnn, case, w, t.Y, max_batch=B)
        s = gnn.Sampler(n, seed=1)
        g.train_range(0, B, 5, steps, moms)
        if evaluate:
            g.confusion_range(0, n, labels=True)
            g.members[0].confusion_range(0, n)
        g.train_sampled(s, 3, B, steps, moms)
        if evaluate:
            g.confusion_range(0, n)
        g.train_sampled(s, 3, B, steps, moms)
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


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals(gnn, oracle_mod):
    case, t = gc.CASES["E2"], gc.truth(oracle_mod, "E2")
    g = gnn.NetGroup(case.dims, list(range(1, case.K + 1)), inner_act=case.inner)
    with pytest.raises(gnn.GnnError) as e:  # no data set
        g.confusion_range(0, 4)
    assert e.value.code == 5
    for call in (lambda: g.members[0].evaluate_range(0, 4), lambda: g.members[0].confusion_range(0, 4),
                 lambda: g.members[0].labels_range(0, 4)):
        with pytest.raises(gnn.GnnError) as e:
            call()
        assert e.value.code == 5
    with pytest.raises(ValueError):
        g.members[0].confusion_range()      # n=None needs an uploaded data set
    g.close()
    g = _group(gnn, case, _weights(oracle_mod, case), t.Y)
    n, lib, m0 = case.rows, g._lib, g.members[0]
    assert lib.gnn_mlp_group_confusion_range(g._h, 0, 4, None, None, None) == 1      # every output null
    assert lib.gnn_mlp_evaluate_range(m0._h, 0, 4, None, None, None, None) == 1
    for first, cnt in ((0, 0), (0, -3), (-1, 4), (n - 3, 4), (n, 1), (0, n + 1)):    # rows outside the data set
        for call in (lambda: g.confusion_range(first, cnt), lambda: m0.evaluate_range(first, cnt),
                     lambda: m0.confusion_range(first, cnt), lambda: m0.labels_range(first, cnt)):
            with pytest.raises(gnn.GnnError) as e:
                call()
            assert e.value.code == 1
    # single outputs are enough
    h = C.c_int64()
    assert lib.gnn_mlp_evaluate_range(m0._h, 0, n, C.byref(h), None, None, None) == 0
    assert h.value == m0.count_hits_range(0, n)
    s = C.c_double()
    assert lib.gnn_mlp_evaluate_range(m0._h, 0, n, None, C.byref(s), None, None) == 0
    assert s.value == m0.evaluate_range(0, n)[1]
    g.close()
