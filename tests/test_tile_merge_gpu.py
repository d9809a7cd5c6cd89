"""The tile kernel's training launch on the merged map (csrc/tile_step_kernel.h: make_merged_tile_map; tile_step_body.inc: a
group of layer 0's partial last tile row, a pair of a later layer, in ONE workgroup) against the same calls with
GNN_MLP_TILE_MERGE=0 (one tile per workgroup).  Merging changes which workgroup computes a tile and not one operation of the
tile's sums or their order, so weights and momentum are compared with np.array_equal: no tolerance.

What runs here: three small shapes and the headline one (a 16-row partial row in groups of 4 + 3, a 32-row one in groups of 2 + 1,
a later layer's 48-row partial tile row), batches of 128, 100, 16 and 144 rows, SoftmaxCrossEntropyNeuralNet with its default
activation, train_range and one NeuralNetTrainer.  The other geometries, batch sizes, call forms and net classes, and the
comparison with the fp64 oracle, are in tests/test_tile_merge_cases_gpu.py."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
STEPS = 6
# 80 = 64 + 16 weight rows: a 16-high partial row of 7 columns (groups of 4 + 3), later layers of 3 and 1 columns, two tile rows in
# layer 1; 96 = 64 + 32: a 32-high partial row of 3 columns (groups of 2 + 1); five layers (its 48-high last row stays whole)
SHAPES = [[80, 112, 48, 10], [96, 48, 32, 10], [100, 64, 48, 32, 10]]
# a whole K chunk; ragged (not a multiple of 16); one 16-row block; a second K chunk (on a handle with max_batch 144)
BATCHES = [128, 100, 16, 144]


def data(dims, n, seed):
    rng = np.random.default_rng(seed)
    X = rng.random((n, dims[0])) * (rng.random((n, dims[0])) < 0.3)
    Y = np.eye(dims[-1])[rng.integers(0, dims[-1], n)]
    return X, Y


def merge_state(net):
    return net.tile_merge_state


def pair(monkeypatch, make, merged=True):
    """make() as it is by default and with GNN_MLP_TILE_MERGE=0 (read once at create)."""
    if os.environ.get("GNN_MLP_PATH") or os.environ.get("GNN_MLP_CHAIN") == "0" or os.environ.get("GNN_MLP_ROWBLOCK") == "0" \
            or os.environ.get("GNN_MLP_TILE_HEAD") or os.environ.get("GNN_MLP_TILE_MERGE"):
        pytest.skip("path forced by the environment")
    new = make()
    monkeypatch.setenv("GNN_MLP_TILE_MERGE", "0")
    old = make()
    monkeypatch.delenv("GNN_MLP_TILE_MERGE")
    assert new.step_launches == old.step_launches and (new.step_launches == 2 or not merged)
    assert merge_state(old) == 0
    assert (merge_state(new) > 0) == merged     # the default build really runs the merged kinds (or, too large a net, does not)
    return new, old


def same(new, old):
    assert np.array_equal(new.get_weights(), old.get_weights())
    assert np.array_equal(new.get_momentum(), old.get_momentum())


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("dims", SHAPES, ids=lambda d: "-".join(map(str, d)))
def test_train_range_bitwise_and_however_it_is_cut(gnn, monkeypatch, dims, B):
    X, Y = data(dims, 3 * B, seed=B)
    new, old = pair(monkeypatch, lambda: gnn.SoftmaxCrossEntropyNeuralNet(dims, max_batch=B))
    cut = pair(monkeypatch, lambda: gnn.SoftmaxCrossEntropyNeuralNet(dims, max_batch=B))[0]
    single = pair(monkeypatch, lambda: gnn.SoftmaxCrossEntropyNeuralNet(dims, max_batch=B))[0]
    for net in (new, old, cut, single):
        net.upload_dataset(X, Y)
    for net in (new, old):
        net.train_range(0, B, STEPS, 0.0125, 0.9)       # (the loop announces every step's successor: <1, 2, true>)
    same(new, old)
    assert np.any(new.get_momentum() != 0)
    # the same steps in calls of 2 + 1 + 3: a call's last step has no successor (the one-tile form without a forward half), the
    # next call starts from a forward-only launch's slabs
    s = 0
    for n in (2, 1, 3):
        cut.train_range((s % 3) * B, B, n, 0.0125, 0.9)
        s += n
    same(cut, old)
    for s in range(STEPS):
        single.train_range((s % 3) * B, B, 1, 0.0125, 0.9)
    same(single, old)


@pytest.mark.parametrize("B", [128, 100])
@pytest.mark.parametrize("dims", SHAPES, ids=lambda d: "-".join(map(str, d)))
def test_train_sampled_with_a_fixed_seed(gnn, monkeypatch, dims, B):
    """The sampled loop: the chain's first step gathers its rows through the index vector, the later ones read the staged copies
    the row-block kernel wrote -- both reach the partial-row group's loads."""
    X, Y = data(dims, 5 * B, seed=11 + B)
    new, old = pair(monkeypatch, lambda: gnn.SoftmaxCrossEntropyNeuralNet(dims, max_batch=B))
    for net in (new, old):
        gnn.NeuralNetTrainer(X, Y, net, seed=3).train(STEPS, 0.0125, B, 0.9)
    same(new, old)
    assert np.any(new.get_momentum() != 0)


def test_forward_only_slabs_start_the_chain(gnn, monkeypatch):
    """A chain that a forward-only launch starts (its slabs come from the one-tile map of layer 0) and the merged kinds go on
    from: after a call of one step, a call of three more, against one call of four and against the one-tile kernels."""
    dims, B = [80, 112, 48, 10], 128
    X, Y = data(dims, 4 * B, seed=5)
    new, old = pair(monkeypatch, lambda: gnn.SoftmaxCrossEntropyNeuralNet(dims, max_batch=B))
    whole = pair(monkeypatch, lambda: gnn.SoftmaxCrossEntropyNeuralNet(dims, max_batch=B))[0]
    for net in (new, old, whole):
        net.upload_dataset(X, Y)
    for net in (new, old):
        net.train_range(0, B, 1, 0.0125, 0.9)
        net.train_range(B, B, 3, 0.0125, 0.9)
    whole.train_range(0, B, 4, 0.0125, 0.9)
    same(new, old)
    same(new, whole)


def test_a_net_with_more_units_than_cus_keeps_the_one_tile_map(gnn, monkeypatch):
    dims, B = [1000, 512, 256, 16], 128
    X, Y = data(dims, 2 * B, seed=9)
    new, old = pair(monkeypatch, lambda: gnn.SoftmaxCrossEntropyNeuralNet(dims, max_batch=B), merged=False)
    for net in (new, old):
        net.upload_dataset(X, Y)
        net.train_range(0, B, STEPS, 0.0125, 0.9)
    same(new, old)


def test_headline_shape_runs_one_workgroup_per_cu(gnn, monkeypatch):
    dims, B = [784, 300, 100, 10], 128
    X, Y = data(dims, 2 * B, seed=1)
    new, old = pair(monkeypatch, lambda: gnn.SoftmaxCrossEntropyNeuralNet(dims, max_batch=B))
    assert merge_state(new) == 256
    for net in (new, old):
        net.upload_dataset(X, Y)
        net.train_range(0, B, STEPS, 0.0125, 0.9)
    same(new, old)
