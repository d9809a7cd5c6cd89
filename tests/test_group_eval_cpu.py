"""The fixtures of the group-evaluation tests (tests/group_eval_cases.py), pinned on the fp64 oracle: a GPU test compares labels
and hits only on rows whose top-2 margin exceeds the project's budgets, so the fixtures must leave few rows below them -- a
test may not pass by declaring rows unsafe -- and the ensemble must predict several classes.  Plus what NetGroup's evaluation
methods refuse before any device call."""
import ctypes as C

import numpy as np
import pytest

from tests import group_eval_cases as gc


@pytest.mark.parametrize("name", gc.NAMES)
def test_fixture_is_decisive(oracle_mod, name):
    case = gc.CASES[name]
    t = gc.truth(oracle_mod, name)
    n = case.rows
    assert t.out.shape == (case.K, n, case.dims[-1])
    unsafe = [int((~t.safe[k]).sum()) for k in range(case.K)] + [int((~t.ens_safe).sum())]
    print(name, "unsafe rows per member, then the ensemble:", unsafe, "of", n)
    assert max(unsafe) <= 0.10 * n
    assert len(set(t.ens_label.tolist())) >= 4
    # the expected rows: even rows the ensemble's label, odd rows (7 r) mod d_out
    assert np.array_equal(t.expected[0::2], t.ens_label[0::2])
    assert np.array_equal(t.expected[1::2], (7 * np.arange(1, n, 2)) % case.dims[-1])
    assert np.isfinite(t.loss).all() and t.loss.shape == (case.K, n)


def test_member_weights_are_f32_values(oracle_mod):
    w = gc.member_weights(oracle_mod, gc.CASES["E2"], 3)
    assert np.array_equal(w, w.astype(np.float32).astype(np.float64))
    assert not np.array_equal(w, gc.member_weights(oracle_mod, gc.CASES["E2"], 4))


def test_null_group_is_refused(gnn):
    """A group object whose handle is null: the three entry points return GNN_ERR_BAD_ARG (or -1 for the launch count)."""
    g = gnn.NetGroup.__new__(gnn.NetGroup)
    g._lib, g._h, g.seeds, g.layer_dims, g.members = gnn.load_library(), C.c_void_p(), [1, 2, 3], [4, 3, 2], []
    assert g.eval_launches == -1
    for call in (lambda: g.evaluate_range(0, 4), lambda: g.ensemble_propagate_range(0, 4), lambda: g.ensemble_argmax_range(0, 4)):
        with pytest.raises(gnn.GnnError) as e:
            call()
        assert e.value.code == 1
    with pytest.raises(ValueError):
        g.evaluate_range()  # n=None needs an uploaded data set
