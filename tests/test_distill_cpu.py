"""The fixtures of tests/test_distill_gpu.py discriminate (tests/distill_cases.py; no GPU): the teacher's rows of the range are
all different, each wrong implementation modelled in numpy leaves the bounds of the group-teacher test by a factor of 100 or
more, the float32 restatement of the blend stays inside them, and smooth_labels is what it says."""
import itertools

import numpy as np
import pytest

from tests import distill_cases as dc

CASES = list(dc.CASES)
DTYPES = [dc.F32, dc.BF16]
BOTH = pytest.mark.parametrize("dt", DTYPES, ids=["f32", "bf16"])


def _mean(oracle_mod, case, dt):
    """The ensemble's mean output on all resident rows, as the device forms it from the (oracle's) member rows."""
    return dc.ensemble_f32(dc.teacher_outputs(oracle_mod, case, dt))


@pytest.mark.parametrize("name", CASES)
@BOTH
def test_no_two_rows_of_the_range_have_the_same_teacher_output(oracle_mod, name, dt):
    case = dc.CASES[name]
    rows = slice(dc.FIRST, dc.FIRST + dc.COUNT)
    for what, t in [("ensemble", _mean(oracle_mod, case, dt)[rows])] + \
                   [("teacher %d" % k, o[rows]) for k, o in enumerate(dc.teacher_outputs(oracle_mod, case, dt))]:
        gap = np.abs(t[:, None, :] - t[None, :, :]).max(axis=2)
        gap[np.arange(dc.COUNT), np.arange(dc.COUNT)] = np.inf
        print("distill fixtures, %s %s %s: smallest row distance %.3g (needs %.3g)" % (name, "bf16" if dt else "f32", what, gap.min(), dc.ROW_GAP))
        assert gap.min() >= dc.ROW_GAP, what
    # ... and the rows next to the range differ from the one-hot rows they must keep by far more than the bound
    assert np.abs(_mean(oracle_mod, case, dt) - dc.onehot(case)).max(axis=1).min() > 100 * dc.BLEND_BOUND


@pytest.mark.parametrize("name", CASES)
@BOTH
@pytest.mark.parametrize("keep", [0.0, dc.KEEP])
def test_every_wrong_implementation_leaves_the_bound(oracle_mod, name, dt, keep):
    case = dc.CASES[name]
    outs = dc.teacher_outputs(oracle_mod, case, dt)
    t = _mean(oracle_mod, case, dt)
    y = dc.onehot(case)
    right = dc.distilled(case, y, t[dc.FIRST:dc.FIRST + dc.COUNT], keep)
    models = {
        "block offset": dc.wrong_block_offset(case, y, t, keep),
        "dense stride for ld": dc.wrong_dense_stride(case, y, t, keep),
        "wrong K": dc.wrong_k(case, y, outs[:, dc.FIRST:dc.FIRST + dc.COUNT], keep),
        "keep swapped": dc.wrong_swapped(case, y, t, keep),
    }
    for what, got in models.items():
        d = np.abs(got - right).max()
        print("distill fixtures, %s %s keep %.2f, %s: %.3g = %.3g bounds" % (name, "bf16" if dt else "f32", keep, what, d, d / dc.BLEND_BOUND))
        assert d >= 100 * dc.BLEND_BOUND, what
    # a fault that touches a neighbour of the range is seen there: the dense-stride model writes below row FIRST + COUNT only,
    # the others nowhere outside -- the untouched rows are compared exactly on the device
    assert np.array_equal(right[:dc.FIRST], y[:dc.FIRST]) and np.array_equal(right[dc.FIRST + dc.COUNT:], y[dc.FIRST + dc.COUNT:])


@pytest.mark.parametrize("name", CASES)
@BOTH
def test_the_float32_restatement_of_the_blend_stays_inside_the_bound(oracle_mod, name, dt):
    case = dc.CASES[name]
    t = _mean(oracle_mod, case, dt)[dc.FIRST:dc.FIRST + dc.COUNT]
    y = dc.onehot(case)[dc.FIRST:dc.FIRST + dc.COUNT]
    assert t.min() >= 0.0 and t.max() <= 1.0            # (the bound is stated for values in [0, 1])
    for keep in (dc.KEEP, 0.1, 0.5, 0.9):
        d = np.abs(dc.blend_f32(y, t, keep) - dc.blend_f64(y, t, float(np.float32(keep)))).max()
        print("distill fixtures, %s %s keep %.2f: float32 blend %.3g = %.3g of the bound" % (name, "bf16" if dt else "f32", keep, d, d / dc.BLEND_BOUND))
        assert d <= dc.BLEND_BOUND
    # the two ends are exact in float32
    assert np.array_equal(dc.blend_f32(y, t, 0.0), t) and np.array_equal(dc.blend_f32(y, t, 1.0), y)


def test_the_range_spans_three_blocks_and_a_ragged_one():
    assert dc.FIRST > 0 and dc.FIRST + dc.COUNT < dc.N
    assert dc.COUNT // dc.BLOCK == 3 and 0 < dc.COUNT % dc.BLOCK < 16
    assert dc.CASES["D10"].ld == 16 and dc.CASES["D20"].ld == 32 and dc.CASES["D20"].d_out % 4 == 0 and dc.CASES["D10"].d_out % 4 != 0


@pytest.mark.parametrize("d_out,eps", itertools.product([2, 10, 20], [0.0, 0.1, 0.3]))
def test_smooth_labels(gnn, d_out, eps):
    labels = np.random.default_rng(3).integers(0, d_out, 50)
    Y = gnn.smooth_labels(labels, d_out, eps)
    assert Y.shape == (50, d_out) and Y.dtype == np.float64
    assert np.allclose(Y.sum(axis=1), 1.0, rtol=0, atol=4e-16 * d_out)
    assert np.array_equal(Y.argmax(axis=1), labels)
    assert np.allclose(Y, (1 - eps) * np.eye(d_out)[labels] + eps / d_out, rtol=0, atol=1e-16)
    with pytest.raises(ValueError):
        gnn.smooth_labels([d_out], d_out, eps)
    with pytest.raises(ValueError):
        gnn.smooth_labels([0], d_out, 1.5)
