"""The reference's label rule (MT:166-168: `>=` scan from actual = 0 -- exact ties to the HIGHEST index, a NaN at an index > 0
never selected, a NaN at index 0 sticky, with softmax any NaN logit gives 0) on every label-writing head of the library.
Fixtures, truth and the fault models these comparisons can see: tests/label_rule_cases.py, pinned by
tests/test_label_rule_cpu.py.  EVERY label is compared, and every hit count and confusion matrix exactly: the fixtures have no
row whose label is unsafe (exact ties by identical columns; the winning group leads by thousands of output budgets).

A ROUTE is a fixture, a dtype and the environment switches that send it to a head; the route assertions are those of
tests/test_saturation_gpu.py (step_launches, rowblock_state, plan_note, specialization):
  two-launch (f32) ................... labels come from middle4_kernel's forward-only instance: its row tail (16-lane row16_argmax)
  two-launch (bf16) .................. per-layer GEMMs + tail_kernel<BF16> (a quad of lanes)
  GNN_MLP_ROWBLOCK=0 ................. middle4_kernel's row tail
  last hidden layer of 132 ........... middle4_kernel's register head
  17 / 40 outputs .................... middle4_kernel's general head (lane c0 scans c0, c0 + 16, ..)
  GNN_MLP_PATH=generic ............... tail_kernel f32 / bf16; with GNN_MLP_TAIL=0 output_layer_kernel's register arm
  300 outputs, GNN_MLP_PATH=generic .. output_layer_kernel's register arm with two 256-column chunks (plan.hip use_tail: the tail
                                       kernel takes a padded width of 16 only; kernels.h: up to 1024 padded outputs in registers)
  1100 outputs ....................... output_layer_kernel's three-pass arm
  GeneralNeuralNet ................... the element-wise arm of each of these heads
  784-100-50-10 ...................... the prebuilt static instances of both net classes (specialization == 1)
  NetGroup ........................... group_forward_kernel's full head (one thread scans a row) and group_combine_kernel's
                                       ensemble scan (eval_launches == 2)
rowblock_body's label arm (quad DPP) is never asked for through the library -- the row-block kernel serves gradients and steps
only (tests/test_saturation_gpu.py says the same of its probabilities) -- so no route reaches it.
Behind the heads: count_hits_kernel, confusion_kernel and group_combine_kernel's hits, through count_hits_range,
evaluate_range and confusion_range (of the data set and of the held-out set).

Tried once on an MI355X: with row16_argmax's step taking the LOWER index on equal values (`oi < ix`), of the 915 GPU tests the
suite had before this file one failed (test_parity_gpu.py::test_argmax_tie_rule), and here the 28 f32 routes whose labels
pass through middle4_kernel failed (row tail, register head, general head, both net classes, the prebuilt instances); the bf16
routes passed, as they must -- a bf16 net's labels come from the per-layer GEMMs and tail_kernel<BF16> / output_layer_kernel."""
import os

import numpy as np
import pytest

from tests import label_rule_cases as lc

pytestmark = pytest.mark.gpu

F32, BF16 = lc.F32, lc.BF16
GENERIC = {"GNN_MLP_PATH": "generic"}
NO_TAIL = {"GNN_MLP_PATH": "generic", "GNN_MLP_TAIL": "0"}
NO_RB = {"GNN_MLP_ROWBLOCK": "0"}
SWITCHES = ("GNN_MLP_PATH", "GNN_MLP_ROWBLOCK", "GNN_MLP_TAIL", "GNN_MLP_CHAIN", "GNN_MLP_STATIC", "GNN_MLP_JIT")

# (fixture, dtype, switches, route): "rb" two launches with the row-block kernel, "m4" two launches with middle4_kernel,
# "gemm" per-layer GEMMs, "static" the prebuilt instances
ROUTES = []
for _n in ("T3", "T4", "T4s", "T16"):
    ROUTES += [(_n, F32, {}, "rb"), (_n, BF16, {}, "rb")]
for _n in ("T3", "T4", "T4s", "T16"):                                    # middle4's row tail
    ROUTES += [(_n, F32, NO_RB, "m4")]
ROUTES += [("T4", BF16, NO_RB, "m4"), ("T16", BF16, NO_RB, "m4")]
for _n in ("T132", "T17", "T40"):                                        # middle4's register head / general head
    ROUTES += [(_n, F32, {}, "m4"), (_n, BF16, {}, "m4")]
for _n in ("T4", "T16"):                                                 # tail_kernel; output_layer_kernel's register arm
    ROUTES += [(_n, F32, GENERIC, "gemm"), (_n, BF16, GENERIC, "gemm"), (_n, F32, NO_TAIL, "gemm"), (_n, BF16, NO_TAIL, "gemm")]
ROUTES += [("T300", F32, GENERIC, "gemm"), ("T300", BF16, GENERIC, "gemm")]   # the register arm, two chunks
ROUTES += [("T1100", F32, {}, "gemm"), ("T1100", BF16, {}, "gemm")]      # the three-pass arm
for _n in ("G_ident", "G_leaky", "G_relu", "G_sigm", "G_tanh"):          # GeneralNeuralNet: the element-wise arm of each head
    ROUTES += [(_n, F32, {}, "rb"), (_n, F32, NO_RB, "m4"), (_n, F32, GENERIC, "gemm"), (_n, BF16, {}, "rb")]
for _n in ("G17_ident", "G17_leaky", "G17_relu", "G17_sigm", "G17_tanh"):
    ROUTES += [(_n, F32, {}, "m4"), (_n, BF16, GENERIC, "gemm")]
for _n in ("TS", "GS"):                                                  # the prebuilt instances, both classes
    ROUTES += [(_n, F32, {}, "static"), (_n, BF16, {}, "static")]


def _route_id(r):
    name, dt, env, route = r
    sw = "".join("-" + k[len("GNN_MLP_"):].lower() + v for k, v in sorted(env.items()))
    return "%s-%s-%s%s" % (name, "bf16" if dt else "f32", route, sw)


def _skip_if_forced(env):
    for k in SWITCHES:
        if k in os.environ and os.environ[k] != env.get(k):
            pytest.skip("%s forced by the environment" % k)


def _make(gnn, monkeypatch, fx, dt, env, route):
    with monkeypatch.context() as m:
        for k, v in env.items():
            m.setenv(k, v)
        if fx.out_kind == lc.SCE:
            net = gnn.SoftmaxCrossEntropyNeuralNet(fx.dims, inner_act=fx.inner, dtype=dt, max_batch=fx.rows)
        else:
            net = gnn.GeneralNeuralNet(fx.dims, inner_act=fx.inner, last_act=fx.last, dtype=dt, max_batch=fx.rows)
    if route == "static":
        assert net.specialization == 1 and net.rowblock_state == 2, "a BASELINE shape must take the prebuilt instances"
    else:
        assert net.specialization == 0
    if route == "rb":
        assert net.step_launches == 2 and net.rowblock_state >= 1, (net.step_launches, net.rowblock_state, net.plan_note)
        assert net.plan_note == ""
    elif route == "m4":
        assert net.step_launches == 2 and net.rowblock_state == 0, (net.step_launches, net.rowblock_state, net.plan_note)
    elif route == "gemm":
        assert net.step_launches == 0 and net.rowblock_state == 0 and net.plan_note != "", (net.step_launches, net.plan_note)
        if "GNN_MLP_PATH" not in env:     # the three-pass arm: more than 1024 padded outputs, which no one-launch kernel takes
            assert (fx.dims[-1] + 15) // 16 * 16 > 1024
        elif fx.out_kind == lc.SCE and fx.dims[-1] > 16:   # the register arm in two chunks
            assert 256 < (fx.dims[-1] + 15) // 16 * 16 <= 512
    net.set_weights(fx.w)
    assert np.array_equal(net.get_weights(), fx.w)
    return net


def _assert_premise(what, fx, out):
    """The outputs of a tie group's columns are bit-equal on every row without a NaN.  Reported apart from the rule."""
    ok = ~np.isnan(out).any(axis=1)
    for g in fx.groups:
        same = (out[ok][:, list(g)] == out[ok][:, [g[0]]]).all(axis=1)
        assert same.all(), ("THE FIXTURE'S PREMISE broke, not the label rule: %s: columns %r of propagate() differ in rows %r"
                            % (what, g, np.flatnonzero(ok)[~same].tolist()))


def _assert_labels(what, got, want):
    bad = np.flatnonzero(np.asarray(got) != want)
    assert bad.size == 0, "%s: rows %r give %r, the rule gives %r" % (what, bad.tolist(), np.asarray(got)[bad].tolist(), want[bad].tolist())


def _assert_resident(what, net, fx, t, order=None):
    """argmax_range, labels_range, count_hits_range, evaluate_range's hits and confusion_range on the uploaded rows."""
    n = fx.rows
    label = t.label if order is None else t.label[order]
    _assert_labels(what + " argmax_range", net.argmax_range(0, n), label)
    _assert_labels(what + " labels_range", net.labels_range(), label)
    if n > 7:                                # a range that starts and ends inside a 4-row block
        _assert_labels(what + " labels_range(3, n - 5)", net.labels_range(3, n - 5), label[3:n - 2])
    assert net.count_hits_range() == t.hits, (what, net.count_hits_range(), t.hits)
    assert net.evaluate_range()[0] == t.hits, what
    conf = net.confusion_range()
    assert np.array_equal(conf, t.conf), "%s: confusion matrix\n%r\nthe rule gives\n%r" % (what, conf, t.conf)


@pytest.mark.parametrize("r", ROUTES, ids=[_route_id(r) for r in ROUTES])
def test_label_rule(gnn, oracle_mod, monkeypatch, r):
    name, dt, env, route = r
    _skip_if_forced(env)
    fx = lc.fixture(oracle_mod, name)
    t = fx.truth(dt)
    n, X, Y = fx.rows, fx.X, fx.Y
    net = _make(gnn, monkeypatch, fx, dt, env, route)
    _assert_premise(_route_id(r), fx, net.propagate(X))
    _assert_labels("argmax on host rows", net.argmax(X), t.label)
    net.upload_dataset(X, Y)
    _assert_resident("resident rows", net, fx, t)
    # the held-out set (the rows moved up by one): what count_hits_range(held_out=True) and the held-out loop's `hits` rule read
    perm = np.r_[1:n, 0]
    net.upload_held_out(X[perm], Y[perm])
    _assert_labels("held-out rows", net.labels_range(held_out=True), t.label[perm])
    assert net.count_hits_range(held_out=True) == t.hits and np.array_equal(net.confusion_range(held_out=True), t.conf)
    # the column-NaN variants
    for v in fx.nan_cols:
        net.set_weights(fx.variant(v))
        tv = fx.truth(dt, v)
        _assert_labels("variant %s, argmax on host rows" % v, net.argmax(X), tv.label)
        _assert_resident("variant %s" % v, net, fx, tv)
    # the rows moved up by one (row 0 last): every 4-row block and 16-row group holds other rows -- the same label per row
    net.set_weights(fx.w)
    net.upload_dataset(X[perm], Y[perm])
    _assert_labels("moved rows, argmax on host rows", net.argmax(X[perm]), t.label[perm])
    _assert_resident("moved rows", net, fx, t, perm)
    net.close()


GROUPS_F = [(n, d) for n in lc.GROUP_NAMES for d in (F32, BF16)]


def _assert_group(what, g, members, dt, nan_member=None):
    fx = members[0]
    n = fx.rows
    ts = [m.truth(dt, "nan" if k == nan_member else None) for k, m in enumerate(members)]
    _, ens_label, ens_hits, ens_conf = lc.ensemble_truth(members, dt, nan_member)
    hits, _, e_hits = g.evaluate_range(0, n)
    conf, e_conf, lab = g.confusion_range(0, n, labels=True)
    for k, t in enumerate(ts):
        _assert_labels("%s member %d" % (what, k), lab[k], t.label)
        assert hits[k] == t.hits, (what, k, hits[k], t.hits)
        assert np.array_equal(conf[k], t.conf), (what, k)
    _assert_labels(what + " ensemble", g.ensemble_argmax_range(0, n), ens_label)
    assert e_hits == ens_hits, (what, e_hits, ens_hits)
    assert np.array_equal(e_conf, ens_conf), what
    return ens_label


@pytest.mark.parametrize("name,dt", GROUPS_F, ids=["%s-%s" % (n, "bf16" if d else "f32") for n, d in GROUPS_F])
def test_label_rule_in_a_group(gnn, oracle_mod, name, dt):
    """Three members with the same tie groups and selectors and different seeds for the rest: the members' labels, hits and
    confusion tables, and those of the ensemble -- the `>=` scan of the member-order f32 mean, whose ties are exact because each
    member's duplicate columns are.  The fixture's NaN input rows give 0 in every member and in the ensemble; with a NaN
    weight in member 1 alone, all of that member's rows and all of the ensemble's are 0."""
    for k in SWITCHES:
        if k in os.environ:
            pytest.skip("%s forced by the environment" % k)
    members = [lc.fixture(oracle_mod, name, seed) for seed in lc.GROUP_SEEDS]
    fx = members[0]
    g = gnn.NetGroup(fx.dims, seeds=list(lc.GROUP_SEEDS), inner_act=fx.inner, dtype=dt, max_batch=fx.rows)
    for k, m in enumerate(members):
        g.members[k].set_weights(m.w)
    g.upload_dataset(fx.X, fx.Y)
    assert g.eval_launches == 2
    mean = g.ensemble_propagate_range(0, fx.rows)
    _assert_premise("the ensemble mean of %s" % name, fx, mean)
    for k, m in enumerate(members):
        _assert_premise("member %d of %s" % (k, name), m, g.members[k].propagate(fx.X))
    ens = _assert_group("group", g, members, dt)
    nan_rows = fx.regime == lc.R_NAN
    assert np.isnan(mean[nan_rows]).all() and (ens[nan_rows] == 0).all() and (ens[~nan_rows] != 0).all()
    g.members[1].set_weights(members[1].variant("nan"))
    ens = _assert_group("member 1 with a NaN weight", g, members, dt, nan_member=1)
    assert (ens == 0).all()
    assert g.eval_launches == 2
    g.close()
