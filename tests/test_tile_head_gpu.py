"""The tile kernel's head-argument prologue (csrc/tile_step_kernel.h: GNN_TS_HEAD_PARAMS, ts_head_tile; W and V requested
behind the first barrier) against the prologue it replaces (GNN_MLP_TILE_HEAD=0: every argument from the struct, every tile
from the lookup, W and V at the top).  Neither changes a floating-point operation or its order, so weights and momentum
are compared with np.array_equal: no tolerance."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
STEPS = 5


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


# (shape, batch): a whole chunk with a clipped rectangle (the `interior` path); a ragged batch (the guarded path); five
# layers; 13 tile rows with K < 128
CASES = [([200, 48, 10], 128), ([300, 40, 10], 17), ([100, 64, 48, 32, 10], 40), ([784, 100, 50, 10], 32)]


@pytest.mark.parametrize("dims,B", CASES)
def test_train_range_bitwise_against_the_earlier_prologue(gnn, monkeypatch, dims, B):
    X, Y = data(dims, 3 * B, seed=B)
    new, old = pair(monkeypatch, lambda: gnn.SoftmaxCrossEntropyNeuralNet(dims, max_batch=B))
    assert new.step_launches == 2 and old.step_launches == 2
    for net in (new, old):
        net.upload_dataset(X, Y)
        net.train_range(0, B, STEPS, 0.0125, 0.9)       # (the loop announces every step's successor: <1, 2, true>)
    same(new, old)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_both_dtypes_on_the_clipped_shape(gnn, monkeypatch, dtype):
    dims, B = [200, 48, 10], 128
    dt = gnn.DTYPE_BF16 if dtype == "bf16" else gnn.DTYPE_F32
    X, Y = data(dims, 3 * B, seed=7)
    new, old = pair(monkeypatch, lambda: gnn.SoftmaxCrossEntropyNeuralNet(dims, max_batch=B, dtype=dt))
    for net in (new, old):
        net.upload_dataset(X, Y)
        net.train_range(0, B, STEPS, 0.0125, 0.9)
    same(new, old)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_train_sampled_with_a_fixed_seed(gnn, monkeypatch, dtype):
    """The sampled loop: the chain's first step gathers its rows through the index vector, the later ones read the staged copies."""
    dims, B = [200, 48, 10], 128
    dt = gnn.DTYPE_BF16 if dtype == "bf16" else gnn.DTYPE_F32
    X, Y = data(dims, 5 * B, seed=11)
    new, old = pair(monkeypatch, lambda: gnn.SoftmaxCrossEntropyNeuralNet(dims, max_batch=B, dtype=dt))
    for net in (new, old):
        gnn.NeuralNetTrainer(X, Y, net, seed=3).train(STEPS, 0.0125, B, 0.9)
    same(new, old)


@pytest.mark.parametrize("rs", [False, True], ids=["direct", "direct_rs"])
def test_two_shared_device_replicas_with_the_direct_reducer(gnn, monkeypatch, rs):
    """The GSRC 2-4 forms: the reduction, the update and the next slabs in the tile kernel of two replicas that share device 0."""
    dims, B = [200, 48, 10], 128
    X, Y = data(dims, 3 * B, seed=13)
    red = gnn.REDUCE_DIRECT_RS if rs else gnn.REDUCE_DIRECT
    new, old = pair(monkeypatch, lambda: gnn.DataParallelNeuralNet(dims, devices=[0, 0], max_batch=B, reducer=red))
    for net in (new, old):
        net.upload_dataset(X, Y)
        net.train_range(0, B, STEPS, 0.0125, 0.9)
        net.synchronize()
        assert net.replicas_identical()
    same(new, old)
