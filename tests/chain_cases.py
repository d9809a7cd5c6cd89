"""The seeded draw of nets, batch sizes and data sets that the chained-loop tests share (tests/test_chain_cases_cpu.py pins its
properties; tests/test_chain_shapes_gpu.py and tests/test_group_gpu.py run it on the device).

A case is a net whose input width sits at an edge of the first-layer K slabs (64 input neurons each; 16 slabs = 1024 inputs is
the last width the two-launch step takes -- plan_chain, MID4_MAX_SLABS) or anywhere below it, 3 to 6 layers, either NeuralNet
class, a batch size that is mostly NOT a multiple of the 4-row blocks / 16-row padding, and a data set of five batches and a
remainder: a sampler over it refills in the middle of a batch within 24 draws (a shortened batch), and a walk over its
contiguous batches wraps."""
import numpy as np

N_CASES = 24
EDGE_D0 = [1, 63, 64, 65, 784, 1023, 1024, 1025]   # one slab; either side of a slab boundary; MNIST's; 16 slabs' last width, the first beyond
LAST_ACTS = [1, 2, 4]                               # sigmoid, tanh, identity (GeneralNeuralNet's last activation)
OUT_SOFTMAX_CE, OUT_ACT_LOSS = 0, 1
STEP, MOMENTUM, ITERATIONS, SAMPLER_SEED = 0.0125, 0.9, 24, 1
W_SCALE = 0.5                                       # start weights = the Random(1) draw times this (keeps f32 softmax inside tolerance)
PAD = 16                                            # batch rows are padded to a multiple of 16, four rows per row-block workgroup


def chain_case(seed):
    """dims, B, inner_act, out_kind, last_act of case `seed` (0..23).

    Widths: d1 in [1, 400), further hidden widths in [1, 130), outputs in [2, 40).  The training row-block kernel
    (rowblock_kernel.h, make_rb_plan) -- and with it every grouped launch (group.hip) -- applies only to nets with at most 16
    outputs and a last hidden layer of at most 128 neurons; drawn from the full ranges 2 of 24 nets meet that and none of those
    has the 3 or 4 layers its bf16 form needs.  So the EVEN seeds draw their last hidden width from [1, 129) and their output
    width from [2, 17); the odd seeds keep the full ranges (middle4_kernel as the two-launch step's row kernel, wide outputs)."""
    rng = np.random.default_rng(7000 + seed)
    L = int(rng.integers(3, 7))
    d0 = EDGE_D0[seed] if seed < len(EDGE_D0) else int(rng.integers(1, 1025))
    narrow = seed % 2 == 0
    hidden = [int(rng.integers(1, 129 if narrow and i == L - 3 else 400 if i == 0 else 130)) for i in range(L - 2)]
    dims = [d0] + hidden + [int(rng.integers(2, 17 if narrow else 40))]
    B = int(rng.integers(1, 70))
    inner = int(rng.integers(0, 4))
    out_kind = OUT_ACT_LOSS if seed % 3 == 2 else OUT_SOFTMAX_CE
    last = LAST_ACTS[int(rng.integers(0, 3))]
    return dims, B, inner, out_kind, last


def dataset_rows(B):
    """Five batches, half a batch and one row."""
    return 5 * B + B // 2 + 1


def chain_data(seed, dims, B):
    """X (half of the entries zero) and one-hot Y of the case's data set."""
    N = dataset_rows(B)
    rng = np.random.default_rng(seed)
    X = rng.random((N, dims[0])) * (rng.random((N, dims[0])) < 0.5)
    Y = np.eye(dims[-1])[rng.integers(0, dims[-1], N)]
    return X, Y


def rowblock_grid(B):
    """Workgroups of the row-block kernel for a batch of B rows."""
    return (B + PAD - 1) // PAD * PAD // 4


def range_batches(N, B, first, n_steps):
    """First rows of the batches train_range(first, B, n_steps) walks over a data set of N rows."""
    nb = N // B
    return [((first // B + s) % nb) * B for s in range(n_steps)]


def oracle_net(oracle_mod, seed):
    """The case's net in the fp64 C oracle with the case's start weights; returns (net, start weights)."""
    dims, B, inner, out_kind, last = chain_case(seed)
    ref = oracle_mod.OracleNet(dims, out_kind=out_kind, inner_act=inner, last_act=last)
    ref.set_alloc_per_sample(0)
    w0 = ref.get_weights().astype(np.float32).astype(np.float64) * W_SCALE   # (the product holds f32 masters: the halved f32 draw is exact in both)
    ref.set_weights(w0)
    return ref, w0


def sampled_draws(oracle_mod, N, B, n=ITERATIONS):
    """The index vectors the reference's sampler (NNT:143-168, Random(1)) hands out in n draws of B from N rows."""
    smp = oracle_mod.Sampler(N, seed=SAMPLER_SEED)
    return [smp.sample(B) for _ in range(n)]


def hinted_walk(N, B, n_steps=20):
    """(first row, rows) of n_steps resident batches that start anywhere in the data set (not at a multiple of B), every fourth
    one a few rows short of B; and for every step but the last the batch a caller announces before it -- the one that follows,
    except at every third step, where the announcement names another batch (and must then go unused)."""
    walk = []
    for s in range(n_steps):
        n = B if s % 4 else max(1, B - 1 - s // 4)
        walk.append(((s * (B + 3)) % (N - B + 1), n))
    hints = [walk[s + 1] if s % 3 != 1 else walk[(s + 2) % n_steps] for s in range(n_steps - 1)]
    return walk, hints
