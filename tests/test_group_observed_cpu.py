"""The observed training loop of a net group (gnn_mlp_group_train_sampled_observed) without a GPU: the interface is there, and the
fixtures of tests/test_group_observed_gpu.py can tell a right curve from a wrong one -- pinned on the fp64 oracle, in units of
the budget (beta) of tests/group_observed_cases.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import chain_cases as cc
from tests import group_observed_cases as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gnn_mlp_group_train_sampled_observed", "gnn_mlp_group_observed_launches")


def test_header_declares_and_library_exports_the_observed_loop(gnn):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gnn_mlp.h")).read(), flags=re.S)
    lib = ctypes.CDLL(gnn.lib_path())
    bound = {n for n, _, _ in gnn._capi.SYMBOLS}
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert hasattr(lib, name), name
        assert name in bound
    assert lib.gnn_mlp_group_observed_launches(None) == -1
    assert hasattr(gnn.NetGroup, "train_sampled_observed") and isinstance(gnn.NetGroup.observed_launches, property)
    assert gnn.NetGroupTrainer.OBSERVER_BURST == gnn.NeuralNetTrainer.OBSERVER_BURST


def test_the_case_lists_are_those_of_the_group_tests():
    from tests import test_group_gpu as tg
    assert oc.GROUPED_CASES == tg.GROUPED_CASES and oc.FALLBACK_CASES == tg.FALLBACK_CASES
    assert oc.case_hyper(5) == tg._case_hyper(5)
    # V = N - 3 lies inside the data set and is ragged in tiles of 32 rows (once a whole pair of them); seeds 0 and 12 have fewer
    # than three tiles, the others up to nine
    vs = {}
    for seed, _, _ in oc.GROUPED_CASES + oc.MEMBER_ROUTE_CASES:
        B = cc.chain_case(seed)[1]
        vs[seed] = oc.validation_rows(B)
        assert 1 <= vs[seed] <= cc.dataset_rows(B) and B < cc.dataset_rows(B)
    assert vs[0] < 96 and vs[12] == 64 and sum(v % 32 != 0 for v in vs.values()) >= len(vs) - 1 and max(vs.values()) > 256
    B = cc.chain_case(oc.REFILL_CASE[0])[1]
    assert oc.REFILL_V <= cc.dataset_rows(B) and oc.REFILL_ITERATIONS > 256 > 16 + 32 + 64 + 128


def test_oracle_fixture_discriminates(oracle_mod):
    """Swapped members, or a curve shifted by one iteration, cannot pass the oracle comparison on the GPU: in the fp64 oracle any
    two members lie >= 74 budgets apart at every iteration at V = 7 (>= 3.2 at V = 150, > 10 at 11 of 12), and a member's
    consecutive values > 5 apart at 9 of 11 pairs at V = 7 (>= 7.5 at all 11 at V = 150)."""
    curves = oc.oracle_curves(oracle_mod)
    m7, s7 = oc.separation(curves[7])
    m150, s150 = oc.separation(curves[150])
    print("V = 7: members", m7.round(1).tolist(), "iterations", s7.round(1).tolist())
    print("V = 150: members", m150.round(1).tolist(), "iterations", s150.round(1).tolist())
    assert np.isfinite(curves[7]).all() and np.isfinite(curves[150]).all()
    assert (m7 >= 50).all() and (s7 > 5).sum() >= 8
    assert (m150 >= 3).all() and (m150 > 10).sum() >= 10 and (s150 > 5).all()


@pytest.mark.parametrize("case", oc.GROUPED_CASES, ids=[oc.id_of(c) for c in oc.GROUPED_CASES])
def test_drawn_cases_keep_finite_curves(oracle_mod, case):
    """The first and the last member of every drawn group over the tests' calls at V = N - 3, in the fp64 oracle: finite values
    in a range in which a relative comparison means something."""
    seed, _, K = case
    B = cc.chain_case(seed)[1]
    curves = oc.drawn_oracle_curves(oracle_mod, seed, sorted({0, K - 1}), oc.SEGMENTS, oc.validation_rows(B))
    print(oc.id_of(case), "curve range", curves.min(), curves.max())
    assert np.isfinite(curves).all() and 0.1 < curves.min() and curves.max() < 10


def test_refill_case_keeps_a_finite_curve(oracle_mod):
    seed, _, K = oc.REFILL_CASE
    curves = oc.drawn_oracle_curves(oracle_mod, seed, [0, K - 1], (oc.REFILL_ITERATIONS,), oc.REFILL_V, lone_step=False)
    print("refill case curve range", curves.min(), curves.max())
    assert np.isfinite(curves).all() and 0.1 < curves.min() and curves.max() < 10
