"""The tile kernel's slots that keep the lookup (csrc/tile_step_body.inc, TS_LOOKUP1: the tiles of the later layers and of
layer 0's partial last tile row ask for the map word, the map_in_args flag and layer 1's descriptor in one batch of scalar
loads and take layer 0's descriptor from the head arguments) against the prologue without any of it
(GNN_MLP_TILE_HEAD=0: every argument from the struct, one dependent load after the other).  Which registers a descriptor
arrives in changes no floating-point operation, so weights and momentum are compared with np.array_equal; two cases are
also held against the fp64 oracle."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
STEPS = 3
STEP, MOMENTUM = 0.0125, 0.9
# f32 against fp64 after one step of the 784-input net is held to 1e-5 by smoke(); three chained steps of nets with
# at most 96 inputs accumulate at most three such errors
ORACLE_TOL = 3e-5


def data(dims, n, seed):
    rng = np.random.default_rng(seed)
    X = rng.random((n, dims[0])) * (rng.random((n, dims[0])) < 0.3)
    Y = np.eye(dims[-1])[rng.integers(0, dims[-1], n)]
    return X, Y


def pair(monkeypatch, make):
    """make() with the default prologue and with GNN_MLP_TILE_HEAD=0 (read once at create)."""
    if os.environ.get("GNN_MLP_PATH") or os.environ.get("GNN_MLP_CHAIN") == "0" or os.environ.get("GNN_MLP_TILE_HEAD"):
        pytest.skip("path forced by the environment")
    new = make()
    monkeypatch.setenv("GNN_MLP_TILE_HEAD", "0")
    old = make()
    monkeypatch.delenv("GNN_MLP_TILE_HEAD")
    return new, old


def same(new, old):
    assert np.array_equal(new.get_weights(), old.get_weights())
    assert np.array_equal(new.get_momentum(), old.get_momentum())


# 80-32-16-10: one whole tile row of layer 0, one partial row of 16, tiles of layers 1 AND 2 (the second trip of a layer
# past 1); 96-32-16-10: a partial row of 32.  128: a whole chunk; 16, 100: ragged (the guarded loads); 144: a second chunk.
SMALL = [([80, 32, 16, 10], B) for B in (128, 16, 100, 144)] + [([96, 32, 16, 10], B) for B in (128, 16, 100, 144)]
# the headline shape; 16 x 44 + 11 = 715 tiles, a map that does not fit the kernel arguments (every slot by the table in
# memory, the plan not regular: whole layer-0 tiles take this path too)
LARGE = [([784, 300, 100, 10], 128), ([1000, 700, 10], 32)]


@pytest.mark.parametrize("dims,B", SMALL + LARGE)
def test_train_range_bitwise_against_the_earlier_prologue(gnn, monkeypatch, dims, B):
    X, Y = data(dims, 3 * B, seed=B + dims[0])
    new, old = pair(monkeypatch, lambda: gnn.SoftmaxCrossEntropyNeuralNet(dims, max_batch=B))
    assert new.step_launches == 2 and old.step_launches == 2
    for net in (new, old):
        net.upload_dataset(X, Y)
        net.train_range(0, B, STEPS, STEP, MOMENTUM)
    same(new, old)


@pytest.mark.parametrize("dims,B", [([80, 32, 16, 10], 128), ([96, 32, 16, 10], 100)])
def test_train_range_against_the_oracle(gnn, oracle_mod, dims, B):
    X, Y = data(dims, 3 * B, seed=5)
    net = gnn.SoftmaxCrossEntropyNeuralNet(dims, max_batch=B)
    ref = oracle_mod.OracleNet(dims)
    net.upload_dataset(X, Y)
    net.train_range(0, B, STEPS, STEP, MOMENTUM)
    for s in range(STEPS):
        ref.gradient_step(X[s * B:(s + 1) * B], Y[s * B:(s + 1) * B], STEP, MOMENTUM)
    d = np.abs(net.get_weights() - ref.get_weights()).max()
    print("max |dW| against the oracle after %d steps: %.3g" % (STEPS, d))
    assert d < ORACLE_TOL


def test_single_steps_each_starting_its_own_chain(gnn, monkeypatch):
    """Steps called one by one: every one begins with the forward-only launch (layer 0's tiles alone, the second map)."""
    dims, B = [80, 32, 16, 10], 128
    X, Y = data(dims, 3 * B, seed=17)
    new, old = pair(monkeypatch, lambda: gnn.SoftmaxCrossEntropyNeuralNet(dims, max_batch=B))
    for net in (new, old):
        net.upload_dataset(X, Y)
        for s in range(STEPS):
            net.gradient_step_range(s * B, B, STEP, MOMENTUM)
    same(new, old)


def test_train_sampled_with_a_fixed_seed(gnn, monkeypatch):
    """The sampled loop: rows by index in the chain's first step, the staged copies after it."""
    dims, B = [80, 32, 16, 10], 128
    X, Y = data(dims, 5 * B, seed=11)
    new, old = pair(monkeypatch, lambda: gnn.SoftmaxCrossEntropyNeuralNet(dims, max_batch=B))
    for net in (new, old):
        gnn.NeuralNetTrainer(X, Y, net, seed=3).train(STEPS, STEP, B, MOMENTUM)
    same(new, old)
