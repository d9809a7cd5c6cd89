"""Confusion matrices (NeuralNet.evaluate_range / confusion_range / labels_range, NetGroup.confusion_range, trainer.per_class):
what needs no device -- per_class, the refusals in front of any device call, and that the fixtures the GPU test uses
(tests/group_eval_cases.py) are decisive for it on the fp64 oracle: matrices far from symmetric, so that a swapped row / column
convention cannot pass, and members that predict several classes."""
import ctypes as C

import numpy as np
import pytest

from tests import group_eval_cases as gc

CASES = ["E2", "E3", "E3b", "E4", "E6", "E6c", "E1b", "E7", "E7g"]


def count(expected, labels, d):
    m = np.zeros((d, d), dtype=np.int64)
    np.add.at(m, (np.asarray(expected), np.asarray(labels)), 1)
    return m


def test_per_class_on_a_hand_written_matrix(gnn):
    conf = np.array([[3, 1, 0],    # class 0 expected 4 times: 3 right, once taken for class 1
                     [0, 0, 0],    # class 1 never expected: recall undefined
                     [2, 1, 0]])   # class 2 expected 3 times, never predicted: precision undefined
    recall, precision = gnn.per_class(conf)
    assert recall[0] == 0.75 and np.isnan(recall[1]) and recall[2] == 0.0
    assert precision[0] == 0.6 and precision[1] == 0.0 and np.isnan(precision[2])
    from gnn_amd import trainer
    assert trainer.per_class is gnn.per_class
    with pytest.raises(ValueError):
        gnn.per_class(np.zeros((2, 3)))


def test_null_handles_are_refused(gnn):
    """Objects whose handle is null: every new method returns GNN_ERR_BAD_ARG; n=None needs a data set."""
    net = gnn.NeuralNet.__new__(gnn.NeuralNet)
    net._lib, net._h, net.layer_dims, net.max_batch = gnn.load_library(), C.c_void_p(), [4, 3, 2], 8
    g = gnn.NetGroup.__new__(gnn.NetGroup)
    g._lib, g._h, g.seeds, g.layer_dims, g.members = gnn.load_library(), C.c_void_p(), [1, 2, 3], [4, 3, 2], []
    for call in (lambda: net.evaluate_range(0, 4), lambda: net.confusion_range(0, 4), lambda: net.labels_range(0, 4),
                 lambda: g.confusion_range(0, 4), lambda: g.confusion_range(0, 4, labels=True)):
        with pytest.raises(gnn.GnnError) as e:
            call()
        assert e.value.code == 1
    for call in (net.evaluate_range, net.confusion_range, net.labels_range, g.confusion_range):
        with pytest.raises(ValueError):
            call()
    lib = gnn.load_library()
    assert lib.gnn_mlp_evaluate_range(None, 0, 4, C.byref(C.c_int64()), None, None, None) == 1
    assert lib.gnn_mlp_group_confusion_range(None, 0, 4, None, None, (C.c_int32 * 4)()) == 1


@pytest.mark.parametrize("name", CASES)
def test_fixture_is_decisive_for_confusion(oracle_mod, name):
    """On the oracle's labels: every member's matrix and the ensemble's differ from their transposes by more rows than the
    unsafe rows could account for, and at least 4 classes are predicted.  |C - C^T| summed over the upper triangle counts the
    rows that break the symmetry; one row whose label changes moves two entries of C, so it changes that sum by at most 2."""
    case, t = gc.CASES[name], gc.truth(oracle_mod, name)
    d = case.dims[-1]
    tables = [(t.label[k], t.safe[k]) for k in range(case.K)] + [(t.ens_label, t.ens_safe)]
    for i, (label, safe) in enumerate(tables):
        conf = count(t.expected, label, d)
        assert conf.sum() == case.rows and np.array_equal(conf.sum(axis=1), np.bincount(t.expected, minlength=d))
        asym = int(np.abs(np.triu(conf - conf.T)).sum())
        unsafe = int((~safe).sum())
        print(name, "table", i, "asymmetry", asym, "unsafe", unsafe, "classes", len(set(label.tolist())),
              "off-diagonal", int(conf.sum() - np.trace(conf)))
        assert asym - 2 * unsafe > 0
        assert len(set(label.tolist())) >= 4
