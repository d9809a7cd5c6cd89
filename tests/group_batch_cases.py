"""The fixtures of the group calls with ONE BATCH SIZE PER MEMBER (gnn_mlp_group_train_sampled_sizes; NetGroup.train_sampled with a
sequence as `batch`): tests/test_group_batches_cpu.py shows with the CPU oracle's sampler what they contain,
tests/test_group_batches_gpu.py runs them on the device.

A fixture is (rows N, batches, iterations, sampler seeds, weight seeds); the data come from np.random.default_rng as in
tests/test_group_samplers_gpu.py.  N is small against the batches, so refills (NNT:149-151) fall inside batches, and a batch that
straddles a refill is shortened by the rows it draws twice (NNT:155) -- for ONE member, while the others' batches are whole."""
import numpy as np

# name: (rows N, batches, iterations, sampler seeds, weight seeds)
FIXTURES = {
    # the reference's recorded sweep (logs/trainLog.csv rows 1-3): batch 2 / 4 / 8; 12 + 9 iterations in two calls
    "SWEEP": (19, [2, 4, 8], 21, [1, 2, 3], [1, 2, 3]),
    # 1 row beside 16, 17 (two 16-row pads) and 12 (a ragged 4-row block structure)
    "RAGGED": (37, [1, 16, 17, 12], 14, [1, 2, 3, 4], [1, 2, 3, 4]),
    # one TS_KC chunk of the tile kernels (<= 128 rows) beside two; max_batch 144
    "CHUNKS": (263, [1, 17, 128, 130], 12, [1, 2, 3, 4], [1, 2, 3, 4]),
    # sixteen members, batches 1 .. 16
    "SIXTEEN": (37, list(range(1, 17)), 14, list(range(1, 17)), list(range(1, 17))),
}
SWEEP_CALLS = [12, 9]
SWEEP_STEPS = [0.0042, 0.0075, 0.01]
SWEEP_MOMENTUM = 0.9
TS_KC = 128  # rows per chunk of the tile kernels' gradient product (csrc/tile_step_kernel.h)
PAD = 16     # batch rows are padded to a multiple of 16

# (iteration, member, size) of every batch a refill shortened -- asserted from the oracle in tests/test_group_batches_cpu.py
SHORTENED = {
    "SWEEP": [(2, 2, 7), (7, 2, 7), (9, 2, 6), (14, 2, 7), (16, 2, 7)],
    "RAGGED": [(2, 1, 14), (4, 1, 15), (4, 2, 14), (6, 2, 16), (8, 2, 16), (9, 1, 14), (9, 3, 11), (11, 1, 15), (13, 1, 15), (13, 2, 16)],
    "CHUNKS": [(2, 2, 124), (2, 3, 128), (4, 2, 122), (4, 3, 128), (6, 2, 122), (6, 3, 126), (8, 2, 115), (8, 3, 124), (10, 2, 117), (10, 3, 123)],
    "SIXTEEN": [(2, 13, 12), (2, 14, 13), (2, 15, 15), (3, 9, 9), (4, 8, 8), (4, 14, 14), (4, 15, 15), (5, 6, 6), (5, 12, 12), (5, 13, 13),
                (6, 10, 10), (7, 4, 4), (8, 8, 8), (8, 12, 11), (9, 7, 7), (9, 11, 10), (9, 15, 14), (10, 6, 6), (11, 12, 12), (11, 15, 15),
                (13, 10, 8), (13, 15, 15)],
}


def batch_sizes(oracle_mod, name, iterations=None, skip=0):
    """(iterations, K) live batch sizes the fixture's samplers draw, after `skip` earlier iterations."""
    N, batches, iters, sseeds, _ = FIXTURES[name]
    iterations = iters if iterations is None else iterations
    out = np.empty((iterations, len(batches)), dtype=np.int64)
    for k, (b, seed) in enumerate(zip(batches, sseeds)):
        s = oracle_mod.Sampler(N, seed=seed)
        for _ in range(skip):
            s.sample(b)
        for i in range(iterations):
            out[i, k] = len(s.sample(b))
    return out


def shortened(sizes, batches):
    return [(i, k, int(sizes[i, k])) for i in range(sizes.shape[0]) for k in range(len(batches)) if sizes[i, k] != batches[k]]


def data(n, d_in, d_out, seed=0):
    rng = np.random.default_rng(seed)
    return rng.random((n, d_in)), np.eye(d_out)[rng.integers(0, d_out, n)]


def hyper(k):
    return [0.01 + 0.004 * i for i in range(k)], [0.9 - 0.03 * i for i in range(k)]
