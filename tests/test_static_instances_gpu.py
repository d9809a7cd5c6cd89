"""Every entry of the PREBUILT instance tables (csrc/static_shapes.h over csrc/instances.h): both shapes x the five inner
activations x both net classes x f32 / bf16, as a single net and as a NetGroup of two.  tests/test_general_net_gpu.py reaches
the General-net instances with sigmoid and leaky ReLU only; a wrong table entry is a kernel built for another activation or
output rule running on this net's buffers, which only the numbers show.  Nets, data, calls and budgets:
tests/static_instance_cases.py; against tests/np_oracle.py in fp64 (bf16: the same roundings in fp64)."""
import numpy as np
import pytest

from tests import test_general_net_gpu
from tests.static_instance_cases import ACT_IDS, B, HYPER, IDENT, LAST, SCALE, SHAPES, STEPS, W_ATOL, budgets, dataset, trajectory
from tests.test_general_net_gpu import forced_path

pytestmark = pytest.mark.gpu

assert W_ATOL == test_general_net_gpu.W_ATOL

_expected = {}


def expected(dims, inner, out_kind, bf, k, w0):
    """trajectory(), computed once per (net, member) and shared by the lone-net and the group case."""
    key = (tuple(dims), inner, out_kind, bf, k)
    if key not in _expected:
        _expected[key] = (w0,) + trajectory(dims, inner, out_kind, bf, k, w0)
        for a in _expected[key]:
            a.setflags(write=False)
    assert np.array_equal(_expected[key][0], w0), "fixture: the start weights of one (net, member) differ between two cases"
    return _expected[key][1:]


def check(net, dims, inner, out_kind, bf, k, what):
    X, _ = dataset(dims[0], dims[-1])
    w, v, out = expected(dims, inner, out_kind, bf, k, net.start_w)
    dw = np.abs(net.get_weights() - w).max()
    dv = np.abs(net.get_momentum() - v).max()
    do = np.abs(net.propagate(X[:B]) - out).max()
    w_tol, o_tol = budgets(bf)
    print("static-instance %s: dw %.3g dv %.3g (budget %.3g) out %.3g (budget %.3g)" % (what, dw, dv, w_tol, do, o_tol))
    assert net.time == STEPS
    assert dw <= w_tol and dv <= w_tol and do <= o_tol, (what, dw, dv, do)


def scaled_start(net, inner):
    net.set_weights(net.get_weights() * SCALE[inner])
    net.start_w = net.get_weights()


@pytest.mark.parametrize("grouped", [False, True], ids=["single", "group2"])
@pytest.mark.parametrize("bf", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["softmax", "general"])
@pytest.mark.parametrize("inner", range(5), ids=ACT_IDS)
@pytest.mark.parametrize("dims", SHAPES, ids=["784-300-100-10", "784-100-50-10"])
def test_prebuilt_instance(gnn, dims, inner, kind, bf, grouped):
    out_kind = gnn.OUT_SOFTMAX_CE if kind == "softmax" else gnn.OUT_ACT_LOSS
    dtype = gnn.DTYPE_BF16 if bf else gnn.DTYPE_F32
    what = "%s %s %s %s %s" % ("-".join(map(str, dims)), ACT_IDS[inner], kind, "bf16" if bf else "f32", "group" if grouped else "single")
    X, Y = dataset(dims[0], dims[-1])
    if grouped:
        g = gnn.NetGroup(dims, [1, 2], out_kind=out_kind, inner_act=inner, last_act=LAST if kind == "general" else IDENT, dtype=dtype, max_batch=B)
        nets = g.members
    elif kind == "softmax":
        nets = [gnn.SoftmaxCrossEntropyNeuralNet(dims, inner_act=inner, dtype=dtype, max_batch=B)]
    else:
        nets = [gnn.GeneralNeuralNet(dims, inner_act=inner, last_act=LAST, dtype=dtype, max_batch=B)]
    if not forced_path():
        assert nets[0].specialization == 1 and nets[0].rowblock_state == 2, "a BASELINE shape must take the prebuilt instances"
        assert not grouped or g.launches_per_step == 2
    for n in nets:
        scaled_start(n, inner)
    if grouped:
        g.upload_dataset(X, Y)
        g.train_range(0, B, STEPS, [h[0] for h in HYPER], [h[1] for h in HYPER])
    else:
        nets[0].upload_dataset(X, Y)
        nets[0].train_range(0, B, STEPS, *HYPER[0])
    for k, n in enumerate(nets):
        check(n, dims, inner, out_kind, bf, k, what + " member %d" % k)
    (g if grouped else nets[0]).close()
