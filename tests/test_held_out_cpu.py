"""What the held-out GPU tests lean on, pinned without a GPU: the structure of the fixtures' fp64 curves
(tests/held_out_cases.py), the best-point rule as a plain function (gnn_amd.best_point), gnn_mlp_held_out_points and the
null-handle behaviour of every new entry point (the library loads without a GPU).

The oracle's figures, as the issue states them and as they reproduce here:
  T1   loss 172.4, 165.7, 162.0, 160.7, 160.3, 162.0, .. 178.5: the loss rule picks point 4, the runner-up is 0.25 % higher; the
       hits rule picks point 8 (23 hits, alone).
  T1h  hits 0, then 1 at every point 1..12; losses 16.10, 15.47, 15.16, 15.37, ..: the hits rule picks point 3; smallest top-2
       margin of any row at any point 2.6e-3.
  T2h  3 hits at points 3, 4, 11, 12 with losses 12.416, 12.448, 12.430, 12.292: the hits rule picks point 12, the loss rule
       point 7; smallest margin 1.4e-3.
  T3   the loss rule picks point 4 (158.3), the runner-up is 1.9 % higher; the hits rule picks point 4.
"""
import ctypes as C

import numpy as np
import pytest

from tests import held_out_cases as hc


def _best(gnn, c, rule):
    return gnn.best_point(c.hits, c.loss, rule)


def test_points():
    assert hc.point_iterations() == [10, 20, 30, 40, 50, 60, 70, 80, 90, 100, 110, 120, 123]
    assert len(hc.point_iterations()) == hc.POINTS


@pytest.mark.parametrize("name, best, first_losses", [("T1", 4, [172.4, 165.7, 162.0, 160.7, 160.3, 162.0]), ("T3", 4, None)])
def test_loss_minimum_inside_the_run(gnn, oracle_mod, name, best, first_losses):
    c = hc.curve(oracle_mod, name)
    at = _best(gnn, c, "loss")
    assert at == best and 0 < at < hc.POINTS - 1  # neither the first nor the last point
    assert at == int(np.argmin(c.loss))
    runner_up = np.sort(c.loss)[1]
    gap = (runner_up - c.loss[at]) / c.loss[at]
    print(name, "loss", np.round(c.loss, 3).tolist(), "gap", gap)
    # the f32 loss-sum budget of test_group_eval_gpu.py, 2e-4 relative + 2e-4 per row, cannot close this gap
    assert gap >= 1e-3
    rows = hc.CASES[name].held_rows
    assert runner_up - c.loss[at] > 2 * (2e-4 * runner_up + 2e-4 * rows)
    if first_losses:
        assert np.allclose(c.loss[:len(first_losses)], first_losses, atol=0.05)


def test_t1_figures(gnn, oracle_mod):
    c = hc.curve(oracle_mod, "T1")
    assert abs(c.loss[-1] - 178.5) < 0.05
    assert _best(gnn, c, "hits") == 8 and c.hits[8] == 23 and (c.hits == 23).sum() == 1
    assert hc.curve(oracle_mod, "T3").loss[4] == pytest.approx(158.3, abs=0.05)
    assert _best(gnn, hc.curve(oracle_mod, "T3"), "hits") == 4


def test_t1h_tie_resolved_inside_the_tied_points(gnn, oracle_mod):
    c = hc.curve(oracle_mod, "T1h")
    assert c.hits.tolist() == [0] + [1] * 12
    assert np.allclose(c.loss[1:5], [16.10, 15.47, 15.16, 15.37], atol=0.006)
    tied = np.flatnonzero(c.hits == c.hits.max())
    at = _best(gnn, c, "hits")
    assert at == 3 and len(tied) > 1 and tied[0] < at < tied[-1]  # neither the first nor the last tied point
    # "equal hits, lower loss" replaces the best twice (points 2 and 3), then never again
    replaced = [p for p in range(2, hc.POINTS) if gnn.best_point(c.hits[:p + 1], c.loss[:p + 1], "hits") == p]
    assert replaced == [2, 3]
    assert c.margin.min() >= 1e-3
    assert c.margin.min() == pytest.approx(2.6e-3, abs=1e-4)


def test_t2h_rules_disagree_and_the_last_tied_point_wins(gnn, oracle_mod):
    c = hc.curve(oracle_mod, "T2h")
    tied = np.flatnonzero(c.hits == c.hits.max())
    assert tied.tolist() == [3, 4, 11, 12] and c.hits.max() == 3
    assert np.allclose(c.loss[tied], [12.416, 12.448, 12.430, 12.292], atol=6e-4)
    assert _best(gnn, c, "hits") == 12 == tied[-1]
    assert _best(gnn, c, "loss") == 7
    assert c.margin.min() >= 1e-3
    assert c.margin.min() == pytest.approx(1.4e-3, abs=1e-4)
    # the tie-break itself is safe in f32: the tied losses lie further apart than the loss-sum budget over 9 rows
    srt = np.sort(c.loss[tied])
    assert srt[1] - srt[0] > 2 * (2e-4 * srt[1] + 2e-4 * 9)


@pytest.mark.parametrize("name", ["T1h", "T2h"])
def test_margins_carry_an_f32_run(oracle_mod, name):
    """Five times the f32 probability budget 2e-4 of test_parity_gpu.py: an f32 GPU run counts the oracle's hits."""
    assert (hc.curve(oracle_mod, name).margin >= 1e-3).all()


def test_ragged_variant_refills_inside_intervals(oracle_mod):
    case = hc.CASES["T1r"]
    assert case.train_rows % hc.BATCH != 0
    smp = oracle_mod.Sampler(case.train_rows, seed=hc.SEED)
    sizes = [len(smp.sample(hc.BATCH)) for _ in range(hc.ITERATIONS)]
    short = [i + 1 for i, n in enumerate(sizes) if n < hc.BATCH]
    print("shortened batches at iterations", short)
    assert short and any(i % hc.EVERY != 0 for i in short)


# ---- gnn_amd.best_point on hand-written curves ----------------------------------------------------------------------------------
def test_best_point_strict_improvement_and_ties(gnn):
    bp = gnn.best_point
    assert bp([0, 0, 0], [3.0, 2.0, 1.0], "loss") == 2
    assert bp([0, 0, 0], [1.0, 2.0, 3.0], "loss") == 0
    assert bp([0, 0, 0, 0], [2.0, 1.0, 1.0, 1.5], "loss") == 1          # a tie keeps the earlier point
    assert bp([1, 2, 2, 1], [9.0, 9.0, 9.0, 1.0], "hits") == 1          # equal hits, equal loss: the earlier point
    assert bp([1, 2, 2, 2], [9.0, 5.0, 4.0, 4.0], "hits") == 2          # equal hits, strictly lower loss
    assert bp([3, 2, 2], [9.0, 1.0, 0.5], "hits") == 0                  # fewer hits never win, whatever the loss
    assert bp([5], [7.0], "loss") == 0 and bp([5], [7.0], "hits") == 0
    assert bp([], [], "loss") == -1
    assert bp([1, 2], [1.0, 2.0], 0) == 0 and bp([1, 2], [1.0, 2.0], 1) == 1
    with pytest.raises(ValueError):
        bp([1], [1.0], "accuracy")
    with pytest.raises(ValueError):
        bp([1, 2], [1.0], "loss")


def test_best_point_nan(gnn):
    bp, nan = gnn.best_point, float("nan")
    assert bp([1, 1, 1], [nan, 2.0, nan], "loss") == 1
    assert bp([1, 1, 1], [nan, nan, nan], "loss") == -1                 # never saw a number
    assert bp([1, 1, 1], [nan, nan, nan], "hits") == 0                  # the hits rule always has a best
    assert bp([1, 1, 2], [nan, 1.0, nan], "hits") == 2                  # more hits win with a NaN loss
    assert bp([1, 1], [2.0, nan], "hits") == 0                          # a NaN loss is never lower
    assert bp([1, 1], [nan, 2.0], "hits") == 0                          # ... and nothing is strictly lower than a NaN
    assert bp([0, 0, 0], [3.0, nan, 2.0], "loss") == 2


# ---- the library, without a GPU ------------------------------------------------------------------------------------------------
def test_held_out_points(gnn):
    lib = gnn.load_library()
    assert lib.gnn_mlp_held_out_points(123, 10) == 13
    assert lib.gnn_mlp_held_out_points(5, 1) == 5
    assert lib.gnn_mlp_held_out_points(5, 9) == 1
    assert lib.gnn_mlp_held_out_points(10, 10) == 1
    assert lib.gnn_mlp_held_out_points(2**31 - 1, 1) == 2**31 - 1
    for bad in ((0, 1), (-3, 1), (5, 0), (5, -1), (0, 0)):
        assert lib.gnn_mlp_held_out_points(*bad) == -1


def test_null_handles_are_refused(gnn):
    lib = gnn.load_library()
    BAD = 1
    x, y = np.zeros((2, 3)), np.zeros((2, 2))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    u8 = (C.c_uint8 * 8)()
    i64, f64, i32 = (C.c_int64 * 64)(), (C.c_double * 64)(), (C.c_int32 * 64)()
    assert lib.gnn_mlp_upload_held_out(None, dp(x), dp(y), 2) == BAD
    assert lib.gnn_mlp_upload_held_out_u8(None, u8, u8, 2) == BAD
    assert lib.gnn_mlp_group_upload_held_out(None, dp(x), dp(y), 2) == BAD
    assert lib.gnn_mlp_group_upload_held_out_u8(None, u8, u8, 2) == BAD
    for s in (0, 1, 2):
        assert lib.gnn_mlp_set_rows(None, s) == -1
        assert lib.gnn_mlp_evaluate_set_range(None, s, 0, 2, i64, f64, None, None) == BAD
        assert lib.gnn_mlp_group_evaluate_set_range(None, s, 0, 2, i64, f64, i64) == BAD
        assert lib.gnn_mlp_group_ensemble_set_range(None, s, 0, 2, f64, i32) == BAD
        assert lib.gnn_mlp_group_confusion_set_range(None, s, 0, 2, i64, i64, i32) == BAD
    assert lib.gnn_mlp_train_sampled_held_out(None, None, 5, 2, 0.1, 0.9, 0, 1, 2, 0, i64, f64, i32, None) == BAD
    assert lib.gnn_mlp_group_train_sampled_held_out(None, None, 5, i32, f64, f64, 0, 1, 2, 0, i64, f64, i64, i32, None) == BAD
    assert b"null" in lib.gnn_mlp_last_error()
