"""The fixtures tests/test_static_instances_gpu.py and tests/test_static_instances_cpu.py share: the nets, the data, the calls,
the budgets and the fp64 trajectory.  No GPU and no product code: numpy and tests/np_oracle.py only.

max_batch = B = 6: two 4-row blocks of the row-block kernel, the second ragged (two live rows, two padding rows).  Three
train_range steps over a 12-row dataset (batches 0, 1, 0) and one forward pass.  Budgets: those of
tests/test_general_net_gpu.py for the same calls -- f32 W_ATOL per step for weights and momentum, 2e-5 for outputs; bf16 5e-3
for outputs and 2e-4 for the weights after three steps, and the same 2e-4 for the momentum (a step's weight change IS the
momentum, so its error is no larger than the weights' own).

Start weights are Random(seed) scaled by SCALE[inner].  Identity: 0.1 -- unscaled, the logits of 784-300-100-10 pass 709 and
the reference's un-normalised softmax (SCE:368) is inf / inf, so the fp64 oracle itself returns NaN.  The two kinked
activations: 0.5, not the 0.1 of start_weights() there: with pre-activations that small, a leaky ReLU net run through the ReLU
instance stays inside the bf16 budgets and a wrong table entry would pass.  tests/test_static_instances_cpu.py asserts that
every wrong activation lands at least two budgets away."""
import functools

import numpy as np

from tests import np_oracle

LEAKY, SIGMOID, TANH, RELU, IDENT = range(5)
ACT_IDS = ["leaky", "sigmoid", "tanh", "relu", "identity"]
SCALE = {LEAKY: 0.5, SIGMOID: 1.0, TANH: 1.0, RELU: 0.5, IDENT: 0.1}
SHAPES = [[784, 300, 100, 10], [784, 100, 50, 10]]
B, STEPS = 6, 3
HYPER = [(0.1, 0.9), (0.08, 0.85)]   # (step, momentum) of member k; a lone net takes member 0's
LAST = SIGMOID                       # the General nets' last activation
W_ATOL = 2e-6                        # per step, f32: tests/test_general_net_gpu.py's (the GPU test asserts that it still is)


@functools.lru_cache(maxsize=None)
def dataset(d_in, d_out):
    """2 B rows, as mnist_like() of tests/test_general_net_gpu.py draws them (19 % of the inputs non-zero, one-hot targets)"""
    rng = np.random.default_rng(83)
    X = rng.random((2 * B, d_in)) * (rng.random((2 * B, d_in)) < 0.19)
    Y = np.eye(d_out)[rng.integers(0, d_out, 2 * B)]
    X.setflags(write=False); Y.setflags(write=False)
    return X, Y


def budgets(bf):
    """(weights and momentum after STEPS steps, outputs)"""
    return (2e-4, 5e-3) if bf else (W_ATOL * STEPS, 2e-5)


def trajectory(dims, inner, out_kind, bf, k, w0):
    """(weights, momentum, outputs of rows [0, B)) after the case's calls with member k's step and momentum, in fp64"""
    X, Y = dataset(dims[0], dims[-1])
    X32 = X.astype(np.float32).astype(np.float64)
    step_fn = np_oracle.gradient_step_bf16 if bf else np_oracle.gradient_step
    w, v = w0.copy(), np.zeros_like(w0)
    for s in range(STEPS):
        sl = slice((s % 2) * B, (s % 2 + 1) * B)
        w, v = step_fn(w, v, dims, X32[sl], Y[sl], HYPER[k][0], HYPER[k][1], inner, out_kind, LAST)
    Ws = np_oracle.split(w, dims)
    out = np_oracle.forward_bf16(Ws, X32[:B], inner, out_kind, LAST)[2] if bf else np_oracle.forward(Ws, X32[:B], inner, out_kind, LAST)[1]
    return w, v, out
