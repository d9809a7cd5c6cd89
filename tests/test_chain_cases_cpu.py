"""Pins the properties of the draw in tests/chain_cases.py that the chained-loop GPU tests rely on (no GPU needed), with the
oracle's own sampler -- so that a later edit of the draw cannot quietly lose them."""
import numpy as np
import pytest

from tests import chain_cases as cc
from tests import np_oracle

SEEDS = range(cc.N_CASES)


def test_draw_is_seeded_and_inside_its_ranges():
    for seed in SEEDS:
        dims, B, inner, out_kind, last = cc.chain_case(seed)
        assert (dims, B, inner, out_kind, last) == cc.chain_case(seed)
        L = len(dims)
        assert 3 <= L <= 6 and 1 <= dims[0] <= 1025
        assert 1 <= dims[1] < 400 and all(1 <= d < 130 for d in dims[2:-1]) and 2 <= dims[-1] < 40
        assert 1 <= B < 70 and inner in (0, 1, 2, 3) and last in cc.LAST_ACTS
        assert out_kind == (cc.OUT_ACT_LOSS if seed % 3 == 2 else cc.OUT_SOFTMAX_CE)
        assert cc.dataset_rows(B) // B == 5 or B == 1           # five whole batches: a contiguous walk of 9 or 8 steps wraps


def test_edge_widths_layer_counts_and_both_classes_occur():
    cases = [cc.chain_case(s) for s in SEEDS]
    assert [c[0][0] for c in cases[:8]] == [1, 63, 64, 65, 784, 1023, 1024, 1025]
    assert {len(c[0]) for c in cases} == {3, 4, 5, 6}
    assert {c[3] for c in cases} == {cc.OUT_SOFTMAX_CE, cc.OUT_ACT_LOSS}
    assert {c[2] for c in cases} == {0, 1, 2, 3}
    # the widths of the slab edges at every slab count the path knows: some case beyond 8 slabs that ends inside a slab
    assert sum(1 for c in cases if c[0][0] > 512 and c[0][0] % 64) >= 4


def test_row_block_grids_that_are_not_a_multiple_of_8():
    """A group launch pads a member's row of workgroups to a multiple of 8 and the surplus workgroups return at once
    (rowblock_group_kernel): the draw must hold batches whose grid has such a surplus, small ones among them."""
    ragged = [s for s in SEEDS if cc.rowblock_grid(cc.chain_case(s)[1]) % 8]
    assert len(ragged) >= 12
    assert sum(1 for s in ragged if cc.chain_case(s)[1] <= 16) >= 3
    assert sum(1 for s in SEEDS if cc.chain_case(s)[1] % 4) >= 12    # a last 4-row block with idle rows


def test_row_block_kernel_shapes_occur():
    """At most 16 outputs and a last hidden layer of at most 128 neurons (make_rb_plan's row tail): the shapes the training
    row-block kernel and the grouped launches exist for -- every layer count, both classes, ragged grids, width 1024; and the
    shapes it refuses remain (the odd seeds)."""
    fits = [s for s in SEEDS if cc.chain_case(s)[0][-1] <= 16 and cc.chain_case(s)[0][-2] <= 128]
    assert all(s in fits for s in SEEDS if s % 2 == 0)
    assert {len(cc.chain_case(s)[0]) for s in fits} == {3, 4, 5, 6}
    assert {cc.chain_case(s)[3] for s in fits} == {cc.OUT_SOFTMAX_CE, cc.OUT_ACT_LOSS}
    assert sum(1 for s in fits if len(cc.chain_case(s)[0]) <= 4) >= 4          # (the bf16 form: three and four layers)
    assert sum(1 for s in fits if cc.rowblock_grid(cc.chain_case(s)[1]) % 8) >= 6
    assert cc.chain_case(6)[0][0] == 1024 and 6 in fits
    assert cc.N_CASES - len(fits) >= 8


def test_announced_walk_stays_inside_the_data_set():
    for seed in SEEDS:
        B = cc.chain_case(seed)[1]
        N = cc.dataset_rows(B)
        walk, hints = cc.hinted_walk(N, B)
        assert len(hints) == len(walk) - 1
        assert all(0 <= f and 1 <= n <= B and f + n <= N for f, n in walk + hints)
        assert any(n < B for _, n in walk) and any(f % B for f, _ in walk)
        wrong = [s for s in range(len(hints)) if hints[s] != walk[s + 1]]
        assert 3 <= len(wrong) < len(hints) // 2


@pytest.mark.parametrize("seed", SEEDS)
def test_sampler_shortens_a_batch_and_the_oracles_agree(oracle_mod, seed):
    """24 draws of B from 5 B + B // 2 + 1 rows: the sampler refills inside a batch and the duplicates collapse (NNT:143-168),
    so some batch is shorter than B -- the chain's next_B != B branches.  On those draws the C oracle (sample by sample) and
    the numpy oracle (matrix form) end on the same weights and momentum: 1e-12 of the vector's largest magnitude, the
    agreement tests/np_oracle.py names (element by element it would be a relative bound on weights that pass through zero)."""
    dims, B, inner, out_kind, last = cc.chain_case(seed)
    N = cc.dataset_rows(B)
    X, Y = cc.chain_data(seed, dims, B)
    draws = cc.sampled_draws(oracle_mod, N, B)
    sizes = [len(d) for d in draws]
    assert max(sizes) == B and min(sizes) < B, sizes
    assert all(0 <= i < N for d in draws for i in d)
    ref, w0 = cc.oracle_net(oracle_mod, seed)
    w, v = w0.copy(), np.zeros_like(w0)
    for idx in draws:
        ref.gradient_step(X[idx], Y[idx], cc.STEP, cc.MOMENTUM)
        w, v = np_oracle.gradient_step(w, v, dims, X[idx], Y[idx], cc.STEP, cc.MOMENTUM, inner, out_kind, last)
    wr, vr = ref.get_weights(), ref.get_momentum()
    assert np.isfinite(wr).all() and np.abs(wr).max() < 1.0
    assert np.abs(w - wr).max() <= 1e-12 * np.abs(wr).max()
    assert np.abs(v - vr).max() <= 1e-12 * max(np.abs(vr).max(), 1e-3)
    assert np.abs(wr - w0).max() > 100 * 2e-6 * cc.ITERATIONS     # the trajectory moves the weights far beyond the GPU tests' budget
