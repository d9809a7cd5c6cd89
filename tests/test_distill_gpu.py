"""Targets of resident rows on the device (include/gnn_mlp.h "targets of resident rows"; csrc/distill.hip, csrc/distill_kernel.h):
get_targets / set_targets, propagate_range, and distill_from with a lone teacher and with a group's ensemble.  Fixtures, bounds
and the wrong implementations these comparisons are able to see: tests/distill_cases.py, pinned by tests/test_distill_cpu.py.

Every call works on the middle range [37, 237) of 300 resident rows in blocks of 64 (three full blocks and one of 8 rows), and
both neighbours of the range are compared exactly.

Measured on an MI355X (23 tests, none skipped, 4.2 s for the file), f32 / bf16: the ensemble's output against the fp64 oracle
4.5e-8 and 1.2e-7 (D10, D20) / 7.7e-4 and 1.1e-3; propagate_range 6.2e-8 and 9.7e-8 / 1.5e-3 and 2.0e-3; keep = 0.25 against the
fp64 blend 0.078 (D10) and 0.156 (D20) of the 2^-22 bound in both dtypes, and bit for bit the float32 restatement; W and V after
30 iterations of train_sampled on distilled rows 0.0026 and 1.5e-5 of the bound / 6.5e-4 and 3.4e-6."""
import ctypes as C

import numpy as np
import pytest

from tests import distill_cases as dc
from tests import soft_target_cases as st

pytestmark = pytest.mark.gpu

F32, BF16 = dc.F32, dc.BF16
BOTH = pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
CASES = pytest.mark.parametrize("name", list(dc.CASES))
RANGE = slice(dc.FIRST, dc.FIRST + dc.COUNT)


def _net(gnn, monkeypatch, case, dims, dt, w=None):
    with monkeypatch.context() as m:
        m.setenv("GNN_MLP_EVAL_ROWS", "0")     # blocks of max_batch rows (tests/test_group_eval_gpu.py)
        if case.kind == dc.SCE:
            net = gnn.SoftmaxCrossEntropyNeuralNet(dims, inner_act=case.inner, dtype=dt, max_batch=dc.BLOCK)
        else:
            net = gnn.GeneralNeuralNet(dims, inner_act=case.inner, last_act=case.last, dtype=dt, max_batch=dc.BLOCK)
    if w is not None:
        net.set_weights(w)
    return net


def _student(gnn, oracle_mod, monkeypatch, case, dt, Y=None):
    net = _net(gnn, monkeypatch, case, case.student, dt, dc.student_weights(oracle_mod, case))
    net.upload_dataset(dc.inputs(case), dc.onehot(case) if Y is None else Y)
    return net


def _teachers(gnn, oracle_mod, monkeypatch, case, dt, upload=True):
    with monkeypatch.context() as m:
        m.setenv("GNN_MLP_EVAL_ROWS", "0")
        g = gnn.NetGroup(case.teacher, list(range(1, dc.K + 1)), out_kind=case.kind, inner_act=case.inner, last_act=case.last,
                         dtype=dt, max_batch=dc.BLOCK)
    for k in range(dc.K):
        g.members[k].set_weights(dc.teacher_weights(oracle_mod, case, k))
    if upload:
        g.upload_dataset(dc.inputs(case), dc.onehot(case))
    assert g.eval_launches == (2 if case.grouped else 0)
    return g


def _soft_rows(d_out, rows, seed=11):
    """The six row kinds of tests/soft_target_cases.py (general nets: free values and one-hot rows), f32-exact."""
    rng = np.random.default_rng(seed)
    return st._targets(rng, st.kinds(rows), d_out, np.zeros(rows, dtype=np.int64))


def _state(net):
    return net.get_weights(), net.get_momentum(), net.time


# ---- 1. round trip -------------------------------------------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize("held_out", [False, True], ids=["train", "held-out"])
def test_targets_round_trip(gnn, monkeypatch, dt, held_out):
    case = dc.CASES["D10"]
    net = _net(gnn, monkeypatch, case, case.student, dt)
    rng = np.random.default_rng(5)
    pix = rng.integers(0, 256, (dc.N, case.student[0]), dtype=np.uint8)
    lab = dc.labels(case).astype(np.uint8)
    (net.upload_held_out_u8 if held_out else net.upload_dataset_u8)(pix, lab)
    before = net.get_targets(held_out=held_out)
    assert np.array_equal(before, dc.onehot(case))
    Y = _soft_rows(case.d_out, dc.COUNT)
    assert set(st.kinds(dc.COUNT)) == set(range(st.N_KINDS))
    raw = Y + 1e-9 * np.arange(Y.size).reshape(Y.shape)          # not f32-exact: the conversion rounds
    net.set_targets(raw, first=dc.FIRST, held_out=held_out)
    got = net.get_targets(held_out=held_out)
    assert np.array_equal(got[RANGE], raw.astype(np.float32).astype(np.float64))
    assert np.array_equal(got[:dc.FIRST], before[:dc.FIRST]) and np.array_equal(got[dc.FIRST + dc.COUNT:], before[dc.FIRST + dc.COUNT:])
    assert np.array_equal(net.get_targets(dc.FIRST + 3, 5, held_out=held_out), got[dc.FIRST + 3:dc.FIRST + 8])
    # the other set does not exist, and was not made
    assert (net.dataset_size if held_out else net.held_out_size) == 0
    net.close()


# ---- 2. rewritten targets are the uploaded targets -------------------------------------------------------------------------
@CASES
@BOTH
def test_rewritten_targets_train_as_uploaded_targets(gnn, oracle_mod, monkeypatch, name, dt):
    case = dc.CASES[name]
    Y = _soft_rows(case.d_out, dc.N) if case.kind == dc.SCE else st._targets(np.random.default_rng(12), st.kinds(dc.N, st.GENERAL), case.d_out, None)
    a = _student(gnn, oracle_mod, monkeypatch, case, dt)
    a.set_targets(Y)
    b = _student(gnn, oracle_mod, monkeypatch, case, dt, Y=Y)
    assert np.array_equal(a.get_targets(), b.get_targets())
    for net in (a, b):
        smp = gnn.Sampler(dc.N, seed=1)
        net.train_sampled(smp, 20, 16, st.STEP, st.MOMENTUM)
        smp.close()
    wa, va, ta = _state(a)
    wb, vb, tb = _state(b)
    assert ta == tb == 20 and np.isfinite(wa).all()
    assert np.array_equal(wa, wb) and np.array_equal(va, vb)
    assert not np.array_equal(wa, dc.student_weights(oracle_mod, case))
    a.close()
    b.close()


# ---- 3. the planted pair: a pending look-ahead -------------------------------------------------------------------------------
@BOTH
def test_targets_rewritten_under_a_pending_lookahead(gnn, oracle_mod, monkeypatch, dt):
    case = dc.CASES["D10"]
    B = 32
    Y = np.array(dc.onehot(case))
    Y[64:64 + B] = _soft_rows(case.d_out, B, seed=13)
    a = _student(gnn, oracle_mod, monkeypatch, case, dt)
    twin = _student(gnn, oracle_mod, monkeypatch, case, dt, Y=Y)
    assert a.step_launches == 2, a.plan_note       # the two-launch path: the step's tile kernel prepares the announced batch
    for net in (a, twin):
        net.hint_next_range(64, B)
        net.gradient_step_range(0, B, st.STEP, st.MOMENTUM)
        if net is a:
            net.set_targets(Y[64:64 + B], first=64)
        net.gradient_step_range(64, B, st.STEP, st.MOMENTUM)
    wa, va, ta = _state(a)
    wb, vb, tb = _state(twin)
    assert ta == tb == 2 and np.array_equal(wa, wb) and np.array_equal(va, vb)
    # (the second step read the rewritten rows: one-hot rows there give other weights)
    c = _student(gnn, oracle_mod, monkeypatch, case, dt)
    c.gradient_step_range(0, B, st.STEP, st.MOMENTUM)
    c.gradient_step_range(64, B, st.STEP, st.MOMENTUM)
    assert not np.array_equal(c.get_weights(), wa)
    for net in (a, twin, c):
        net.close()


# ---- 4. group teacher ----------------------------------------------------------------------------------------------------------
@CASES
@BOTH
def test_group_teacher(gnn, oracle_mod, monkeypatch, name, dt):
    case = dc.CASES[name]
    g = _teachers(gnn, oracle_mod, monkeypatch, case, dt)
    teacher_state = [_state(m) for m in g.members]
    t = g.ensemble_propagate_range(dc.FIRST, dc.COUNT)
    assert np.array_equal(t, t.astype(np.float32).astype(np.float64))
    ref = dc.ensemble_f32(dc.teacher_outputs(oracle_mod, case, F32))[RANGE]        # the fp64 oracle's members, for both dtypes
    print("distill, %s %s: ensemble output against the oracle %.3g (bound %.3g)" % (name, "bf16" if dt else "f32", np.abs(t - ref).max(), dc.OUT_BOUND[dt]))
    assert np.abs(t - ref).max() <= dc.OUT_BOUND[dt]
    y0 = dc.onehot(case)

    s = _student(gnn, oracle_mod, monkeypatch, case, dt)
    student_state = _state(s)
    s.distill_from(g, keep=1.0, first=dc.FIRST, n=dc.COUNT)
    assert np.array_equal(s.get_targets(), y0)
    s.distill_from(g, keep=0.0, first=dc.FIRST, n=dc.COUNT)
    got = s.get_targets()
    assert np.array_equal(got[RANGE], t)
    assert np.array_equal(got[:dc.FIRST], y0[:dc.FIRST]) and np.array_equal(got[dc.FIRST + dc.COUNT:], y0[dc.FIRST + dc.COUNT:])
    # keep = 1 on rows that are no longer one-hot: every bit stays
    s.distill_from(g, keep=1.0, first=dc.FIRST, n=dc.COUNT)
    assert np.array_equal(s.get_targets(), got)
    s.close()

    s = _student(gnn, oracle_mod, monkeypatch, case, dt)
    s.distill_from(g, keep=dc.KEEP, first=dc.FIRST, n=dc.COUNT)
    got = s.get_targets()
    err = np.abs(got[RANGE] - dc.blend_f64(y0[RANGE], t, dc.KEEP)).max()
    print("distill, %s %s: keep %.2f against the fp64 blend %.3g = %.3g of the bound" % (name, "bf16" if dt else "f32", dc.KEEP, err, err / dc.BLEND_BOUND))
    assert err <= dc.BLEND_BOUND
    assert np.array_equal(got[RANGE], dc.blend_f32(y0[RANGE], t, dc.KEEP))       # (the kernel's own arithmetic, restated)
    assert np.array_equal(got[:dc.FIRST], y0[:dc.FIRST]) and np.array_equal(got[dc.FIRST + dc.COUNT:], y0[dc.FIRST + dc.COUNT:])
    # nothing else moved: the student's and every teacher's weights, momentum and step count, the teachers' own rows
    for a, b in zip(_state(s), student_state):
        assert np.array_equal(a, b)
    for m, before in zip(g.members, teacher_state):
        for a, b in zip(_state(m), before):
            assert np.array_equal(a, b)
    assert np.array_equal(g.members[0].get_targets(), y0)
    assert np.array_equal(g.ensemble_propagate_range(dc.FIRST, dc.COUNT), t)
    s.close()
    g.close()


@BOTH
def test_group_teacher_needs_no_rows_of_its_own(gnn, oracle_mod, monkeypatch, dt):
    """The teachers read the student's resident inputs: a group that never uploaded a data set distils the same rows."""
    case = dc.CASES["D10"]
    out = []
    for upload in (True, False):
        g = _teachers(gnn, oracle_mod, monkeypatch, case, dt, upload=upload)
        s = _student(gnn, oracle_mod, monkeypatch, case, dt)
        s.distill_from(g, keep=0.0, first=dc.FIRST, n=dc.COUNT)
        out.append(s.get_targets())
        s.close()
        g.close()
    assert np.array_equal(out[0], out[1])


# ---- 5. lone teacher -----------------------------------------------------------------------------------------------------------
@CASES
@BOTH
def test_lone_teacher(gnn, oracle_mod, monkeypatch, name, dt):
    case = dc.CASES[name]
    w = dc.teacher_weights(oracle_mod, case, 0)
    teacher = _net(gnn, monkeypatch, case, case.teacher, dt, w)
    teacher.upload_dataset(dc.inputs(case), dc.onehot(case))
    t = teacher.propagate_range(dc.FIRST, dc.COUNT)
    ref = dc.teacher_outputs(oracle_mod, case, F32)[0][RANGE]                          # the fp64 oracle, for both dtypes
    print("distill, %s %s: propagate_range against the oracle %.3g (bound %.3g)" % (name, "bf16" if dt else "f32", np.abs(t - ref).max(), dc.OUT_BOUND[dt]))
    assert np.abs(t - ref).max() <= dc.OUT_BOUND[dt]
    lab = teacher.labels_range(dc.FIRST, dc.COUNT)
    assert np.array_equal(lab, [int(np.flatnonzero(r >= r.max())[-1]) for r in t])       # the `>=` argmax of these rows
    assert np.abs(teacher.propagate_range(dc.FIRST + 5, 70) - ref[5:75]).max() <= dc.OUT_BOUND[dt]   # other blocks, another ragged end
    before = _state(teacher)
    y0 = dc.onehot(case)
    s = _student(gnn, oracle_mod, monkeypatch, case, dt)
    s.distill_from(teacher, keep=0.0, first=dc.FIRST, n=dc.COUNT)
    got = s.get_targets()
    assert np.array_equal(got[RANGE], t)
    assert np.array_equal(got[:dc.FIRST], y0[:dc.FIRST]) and np.array_equal(got[dc.FIRST + dc.COUNT:], y0[dc.FIRST + dc.COUNT:])
    for a, b in zip(_state(teacher), before):
        assert np.array_equal(a, b)
    assert np.array_equal(teacher.get_targets(), y0)
    # a teacher without rows of its own, and the student as its own teacher
    bare = _net(gnn, monkeypatch, case, case.teacher, dt, w)
    s2 = _student(gnn, oracle_mod, monkeypatch, case, dt)
    s2.distill_from(bare, keep=0.0, first=dc.FIRST, n=dc.COUNT)
    assert np.array_equal(s2.get_targets(), got)
    own = s2.propagate_range(dc.FIRST, dc.COUNT)
    s2.distill_from(s2, keep=dc.KEEP, first=dc.FIRST, n=dc.COUNT)
    assert np.array_equal(s2.get_targets()[RANGE], dc.blend_f32(got[RANGE], own, dc.KEEP))
    # held-out rows through the same call
    teacher.upload_held_out(dc.inputs(case)[RANGE], y0[RANGE])
    assert np.array_equal(teacher.propagate_range(0, dc.COUNT, held_out=True), t)        # the same rows in the same blocks
    for net in (teacher, bare, s, s2):
        net.close()


# ---- 6. the training paths read the new rows ---------------------------------------------------------------------------------
@BOTH
def test_training_reads_the_distilled_rows(gnn, oracle_mod, monkeypatch, dt):
    case = dc.CASES["D10"]
    iterations, batch = 30, 16
    g = _teachers(gnn, oracle_mod, monkeypatch, case, dt, upload=False)
    s = _student(gnn, oracle_mod, monkeypatch, case, dt)
    s.distill_from(g, keep=0.1, first=dc.FIRST, n=dc.COUNT)
    Y = s.get_targets()
    assert not np.array_equal(Y[RANGE], dc.onehot(case)[RANGE]) and np.array_equal(Y[:dc.FIRST], dc.onehot(case)[:dc.FIRST])
    smp = gnn.Sampler(dc.N, seed=1)
    s.train_sampled(smp, iterations, batch, st.STEP, st.MOMENTUM)
    smp.close()
    w, v = dc.oracle_sampled_run(oracle_mod, case, dt, dc.student_weights(oracle_mod, case), dc.inputs(case), Y, iterations, batch,
                                 st.STEP, st.MOMENTUM)
    bound = st.weight_bound(dt, iterations)
    ew, ev = np.abs(s.get_weights() - w).max(), np.abs(s.get_momentum() - v).max()
    print("distill, train_sampled on distilled rows %s: W %.3g V %.3g of the bound %.3g" % ("bf16" if dt else "f32", ew / bound, ev / bound, bound))
    assert s.time == iterations and ew <= bound and ev <= bound
    # the oracle on the one-hot rows ends elsewhere: the comparison sees which rows were read
    w1, _ = dc.oracle_sampled_run(oracle_mod, case, dt, dc.student_weights(oracle_mod, case), dc.inputs(case), dc.onehot(case), iterations,
                                  batch, st.STEP, st.MOMENTUM)
    assert np.abs(w1 - w).max() > 100 * bound
    s.close()
    g.close()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------
def _refused(gnn, code, call, *args, **kw):
    with pytest.raises(gnn.GnnError) as e:
        call(*args, **kw)
    assert e.value.code == code, (e.value.code, str(e.value))
    return str(e.value)


def test_refusals(gnn, oracle_mod, monkeypatch):
    BAD, STATE = 1, 5
    case = dc.CASES["D10"]
    g = _teachers(gnn, oracle_mod, monkeypatch, case, F32)
    teacher = g.members[0]
    s = _student(gnn, oracle_mod, monkeypatch, case, F32)
    before = s.get_targets()
    lib = s._lib
    Y = np.zeros((4, case.d_out))
    yp = Y.ctypes.data_as(C.POINTER(C.c_double))
    # null pointers
    assert lib.gnn_mlp_get_targets_range(None, 0, 0, 4, yp) == BAD and lib.gnn_mlp_get_targets_range(s._h, 0, 0, 4, None) == BAD
    assert lib.gnn_mlp_set_targets_range(None, 0, 0, 4, yp) == BAD and lib.gnn_mlp_set_targets_range(s._h, 0, 0, 4, None) == BAD
    assert lib.gnn_mlp_group_set_targets_range(None, 0, 0, 4, yp) == BAD and lib.gnn_mlp_group_set_targets_range(g._h, 0, 0, 4, None) == BAD
    assert lib.gnn_mlp_propagate_set_range(None, 0, 0, 4, yp) == BAD and lib.gnn_mlp_propagate_set_range(s._h, 0, 0, 4, None) == BAD
    assert lib.gnn_mlp_distill_range(None, teacher._h, 0, 4, 0.5) == BAD and lib.gnn_mlp_distill_range(s._h, None, 0, 4, 0.5) == BAD
    assert lib.gnn_mlp_group_distill_range(None, g._h, 0, 4, 0.5) == BAD and lib.gnn_mlp_group_distill_range(s._h, None, 0, 4, 0.5) == BAD
    # keep outside [0, 1] or NaN
    for keep in (-1e-9, 1.0 + 1e-9, float("nan"), float("inf")):
        _refused(gnn, BAD, s.distill_from, g, keep=keep, first=dc.FIRST, n=dc.COUNT)
        _refused(gnn, BAD, s.distill_from, teacher, keep=keep, first=dc.FIRST, n=dc.COUNT)
    # rows outside the set, a set that is neither value
    for first, n in ((0, 0), (0, -3), (-1, 4), (dc.N - 3, 4), (dc.N, 1), (0, dc.N + 1)):
        _refused(gnn, BAD, s.distill_from, g, keep=0.5, first=first, n=n)
        _refused(gnn, BAD, s.distill_from, teacher, keep=0.5, first=first, n=n)
        _refused(gnn, BAD, s.get_targets, first, n)
        _refused(gnn, BAD, s.propagate_range, first, n)
        assert lib.gnn_mlp_set_targets_range(s._h, 0, first, n, yp) == BAD
        assert lib.gnn_mlp_group_set_targets_range(g._h, 0, first, n, yp) == BAD
    for bad_set in (-1, 2):
        assert lib.gnn_mlp_get_targets_range(s._h, bad_set, 0, 4, yp) == BAD
        assert lib.gnn_mlp_set_targets_range(s._h, bad_set, 0, 4, yp) == BAD
        assert lib.gnn_mlp_group_set_targets_range(g._h, bad_set, 0, 4, yp) == BAD
        assert lib.gnn_mlp_propagate_set_range(s._h, bad_set, 0, 4, yp) == BAD
    # the named set never uploaded
    _refused(gnn, STATE, s.get_targets, 0, 4, held_out=True)
    _refused(gnn, STATE, s.set_targets, Y, held_out=True)
    _refused(gnn, STATE, s.propagate_range, 0, 4, held_out=True)
    _refused(gnn, STATE, g.set_targets, Y, held_out=True)
    bare = _net(gnn, monkeypatch, case, case.student, F32)
    _refused(gnn, STATE, bare.distill_from, g, keep=0.5, first=0, n=4)
    _refused(gnn, STATE, bare.distill_from, teacher, keep=0.5, first=0, n=4)
    # teacher and student differ: the message names which
    wide = _net(gnn, monkeypatch, case, [25, 16, 10], F32)
    assert "dims[0]" in _refused(gnn, BAD, s.distill_from, wide, keep=0.5, first=0, n=4)
    more = _net(gnn, monkeypatch, case, [24, 16, 12], F32)
    assert "dims[L-1]" in _refused(gnn, BAD, s.distill_from, more, keep=0.5, first=0, n=4)
    tanh = gnn.SoftmaxCrossEntropyNeuralNet(case.teacher, inner_act=dc.TANH, max_batch=dc.BLOCK)
    assert "inner activation" in _refused(gnn, BAD, s.distill_from, tanh, keep=0.5, first=0, n=4)
    half = _net(gnn, monkeypatch, case, case.teacher, BF16)
    assert "dtype" in _refused(gnn, BAD, s.distill_from, half, keep=0.5, first=0, n=4)
    gb = _teachers(gnn, oracle_mod, monkeypatch, case, BF16, upload=False)
    assert "dtype" in _refused(gnn, BAD, s.distill_from, gb, keep=0.5, first=0, n=4)
    # hidden layers, depth and output kind may differ
    general = gnn.GeneralNeuralNet([24, 9, 8, 7, 10], inner_act=case.inner, last_act=dc.SIGMOID, max_batch=dc.BLOCK)
    assert np.array_equal(s.get_targets(), before)
    s.distill_from(general, keep=1.0, first=dc.FIRST, n=dc.COUNT)
    # a student that is a member of a group, or a replica of a data-parallel handle; set_targets on a member
    _refused(gnn, STATE, teacher.distill_from, g, keep=0.5, first=0, n=4)
    _refused(gnn, STATE, teacher.distill_from, s, keep=0.5, first=0, n=4)
    msg = _refused(gnn, STATE, teacher.set_targets, Y)
    assert msg == _refused(gnn, STATE, teacher.upload_dataset, dc.inputs(case), dc.onehot(case))
    dp = gnn.DataParallelNeuralNet(case.student, devices=[0, 0], inner_act=case.inner, max_batch=dc.BLOCK, reducer=gnn.REDUCE_DIRECT)
    dp.upload_dataset(dc.inputs(case), dc.onehot(case))
    _refused(gnn, STATE, dp.replicas[0].distill_from, g, keep=0.5, first=0, n=4)
    _refused(gnn, STATE, dp.replicas[1].distill_from, s, keep=0.5, first=0, n=4)
    assert np.array_equal(dp.replicas[0].get_targets(), dc.onehot(case))
    dp.close()
    with pytest.raises(TypeError):
        s.distill_from(object())
    # nothing was written by any of them
    assert np.array_equal(s.get_targets(), before)
    assert np.array_equal(teacher.get_targets(), dc.onehot(case))
    # the group call writes the one copy, which every member reads
    g.set_targets(np.full((4, case.d_out), 0.125), first=dc.FIRST)
    for m in g.members:
        assert np.array_equal(m.get_targets(dc.FIRST - 1, 6)[1:5], np.full((4, case.d_out), 0.125))
        assert np.array_equal(m.get_targets(dc.FIRST - 1, 6)[[0, 5]], dc.onehot(case)[[dc.FIRST - 1, dc.FIRST + 4]])
    for net in (s, bare, wide, more, tanh, half, general):
        net.close()
    gb.close()
    g.close()
