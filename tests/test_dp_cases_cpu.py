"""Pins what tests/test_dp_shapes_gpu.py relies on (no GPU needed): the replica assignment of tests/dp_cases.py meets the
conditions the sweep is for, the Python restatements of the host rules say what csrc/dp.hip says, the invariant behind
tile_step_kernel's owner arithmetic holds on every case, and -- measured on the reference side -- what the f32 budget of the
sweep catches of a WRONG data-parallel step.

Wrong trajectories (fp64 numpy oracle driven along the case's walk, against the fp64 C oracle on the whole batch; budget =
2e-6 per step, the 12 whole-batch steps; the 26 multi-replica cases: 23 drawn + 3 extras).  Cases outside the budget:
    the last replica that has rows dropped from the sum                                  26 of 26  (242 .. 2060 budgets)
    each shard's gradient divided by its own row count, the results averaged             17 of 26
        (the 9 inside, at 1e-12 of the budget, are the cases whose non-empty shards all have the same size: there the rule IS
        the right one -- s0 s3 s7 s11 s12 s16 s20 s21 x1)
    one owner's slice of the flat gradient left as that owner's partial gradient         26 of 26  (the smallest at 1.10 budgets)
    one owner's slice taken from the sum of two steps earlier (the parity buffer)        25 of 26  (s12 stays at 0.35 budgets)
(the owner is the one whose slice holds the most weights)
while the CORRECT sharded trajectory (partial gradients summed in rank order) stays within 1e-9 of the budget.  So the
oracle bound holds most of these, two of them narrowly in some case; what it cannot hold -- a stale slice on s12, an error
confined to a few floats of one tile, a single wrong peer -- is held by the bitwise check of the GPU sweep."""
import numpy as np
import pytest

from tests import chain_cases as cc
from tests import dp_cases as dc
from tests import np_oracle
from tests.test_chain_shapes_gpu import W_ATOL

CASES = range(dc.N_DP_CASES)
DRAWN = range(dc.N_DRAWN)


def _n(i):
    return dc.dp_case(i)[5]


def _B(i):
    return dc.dp_case(i)[1]


def test_the_batches_are_the_ones_the_assignment_was_written_for():
    assert [_B(s) for s in DRAWN] == [15, 13, 50, 11, 24, 62, 19, 42, 26, 27, 41, 48, 12, 55, 38, 15, 34, 44, 37, 21, 46, 21, 38, 53]
    pads = [dc.n_pad(dc.dp_case(s)[0]) for s in DRAWN]
    assert min(pads) == 6400 and max(pads) == 326400
    assert len(dc.REPLICAS) == dc.N_DRAWN and all(1 <= n <= dc.DP_MAX_REPLICAS for n in dc.REPLICAS)


def test_host_rules_restated():
    for B in range(1, 70):
        for n in range(1, 17):
            sizes = dc.shard_sizes(B, n)
            assert sum(sizes) == B and max(sizes) - min(sizes) <= 1 and sizes == sorted(sizes, reverse=True)
            assert sizes.count(max(sizes)) == (B % n or n)
            assert [dc.shard(B, r, n)[0] for r in range(n)] == [sum(sizes[:r]) for r in range(n)]
    assert dc.slice_floats(256, 7) == 48 and dc.slice_floats(6400, 16) == 400 and dc.slice_floats(6401, 16) == 416
    assert dc.n_pad([1, 2]) == 256 and dc.n_pad([784, 300, 100, 10]) == 784 * 304 + 304 * 112 + 112 * 16
    for i in CASES:
        dims = dc.dp_case(i)[0]
        idx = dc.padded_index(dims)
        assert idx.size == sum(a * b for a, b in zip(dims[:-1], dims[1:])) and np.all(np.diff(idx) > 0) and idx[-1] < dc.n_pad(dims)


def test_replica_counts_and_shards():
    ns = [_n(s) for s in DRAWN]
    assert set(ns) == {1, 2, 3, 4, 5, 7, 8, 16}
    assert sum(1 for s in DRAWN if _B(s) < _n(s)) >= 3                                   # replicas without rows
    assert all(_B(s) < 16 for s in DRAWN if _n(s) == 16)
    full = [i for i in CASES if _n(i) == 16 and _B(i) >= 16]                              # ... and 16 replicas that all have rows
    assert full and all(min(dc.shard_sizes(_B(i), 16)) >= 1 and len(dc.dp_case(i)[0]) in (3, 4) for i in full)
    assert sum(1 for s in DRAWN if _B(s) > _n(s) and _B(s) % _n(s)) >= 6                  # unequal shards
    assert any(1 in dc.shard_sizes(_B(s), _n(s)) for s in DRAWN if _B(s) > _n(s))         # a shard of exactly one row
    assert sum(1 for s in DRAWN if _n(s) > 1 and any(k % 4 for k in dc.shard_sizes(_B(s), _n(s)))) >= 12
    assert sum(1 for s in DRAWN if s % 3 == 2 and dc.dp_case(s)[3] == cc.OUT_ACT_LOSS and _n(s) >= 2) >= 4
    assert dc.dp_case(7)[0][0] == 1025 and _n(7) >= 2
    # a next shard that starts at a row which is a multiple of nothing: next_first + lo with lo odd
    assert sum(1 for s in DRAWN if any(dc.shard(_B(s), r, _n(s))[0] % 2 for r in range(_n(s)))) >= 12


def test_reduce_scatter_slices():
    short_last = 0
    for s in DRAWN:
        dims, n = dc.dp_case(s)[0], _n(s)
        if n == 1:
            continue
        offs, npad = dc.layer_offsets(dims)
        sl = dc.slice_floats(npad, n)
        cuts = [k * sl for k in range(1, n) if k * sl < npad]
        assert any(c not in offs for c in cuts), (s, cuts, offs)                          # a boundary strictly inside a matrix
        ranges = [dc.owner_range(npad, n, r) for r in range(n)]
        assert ranges[0][0] == 0 and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:])) and ranges[-1][1] == npad
        live = [hi - lo for lo, hi in ranges if hi > lo]
        short_last += live[-1] < sl
    assert short_last >= 6


def test_the_extras():
    dims, B, inner, out_kind, last, n, _ = dc.dp_case(dc.N_DRAWN)
    assert dims == [1, 2] and n == 7 and dc.n_pad(dims) == 256 and dc.slice_floats(256, 7) == 48
    assert dc.owner_range(256, 7, 5) == (240, 256) and dc.owner_range(256, 7, 6) == (256, 256)
    assert 1 in dc.shard_sizes(B, n) and 2 in dc.shard_sizes(B, n)
    dims, B, inner, out_kind, last, n, _ = dc.dp_case(dc.N_DRAWN + 1)
    assert len(dims) == 3 and max(dims) <= 16 and n == 16 and B == 3
    assert dc.shard_sizes(B, n) == [1, 1, 1] + [0] * 13
    assert out_kind == cc.OUT_ACT_LOSS and last == 4 and inner == 2                       # identity last, tanh inside: neither on a dp handle before
    dims, B, inner, out_kind, last, n, _ = dc.dp_case(dc.N_DRAWN + 2)
    assert n == 16 and B == 17 and dc.shard_sizes(B, n) == [2] + [1] * 15 and len(dims) == 4 and max(dims) <= 64


def test_a_16_float_row_piece_never_straddles_two_owners():
    """dp_handle.h / tile_step_kernel.h, ts_gradient_in<4>: the owner of a lane's 16 B is that of the 16-float row piece they
    lie in.  It holds because every layer offset, every padded row length and the slice are multiples of 16."""
    for i in CASES:
        dims, n = dc.dp_case(i)[0], _n(i)
        offs, npad = dc.layer_offsets(dims)
        sl = dc.slice_floats(npad, n)
        assert sl % 16 == 0 and sl * n >= npad and all(o % 16 == 0 for o in offs) and all(dc.pad16(d) % 16 == 0 for d in dims)
        piece = np.arange(0, npad, 16)
        assert np.array_equal(piece // sl, (piece + 15) // sl)
        assert (npad - 1) // sl <= n - 1                                                  # the last float has an owner
    for npad in range(256, 256 * 40, 256):                                                # and for any buffer made of 16 x 16 blocks
        for n in range(1, 17):
            sl = dc.slice_floats(npad, n)
            assert sl % 16 == 0 and (npad - 1) // sl <= n - 1 and (n - 1) * (sl - 16) < npad


def test_the_walk():
    for i in CASES:
        B, n = _B(i), _n(i)
        N = cc.dataset_rows(B)
        w = dc.walk(B, n)
        assert len(w) == 15 and len(dc.walk(B, n, True)) == 22                            # below a handle's 16th gradient computation; beyond it
        assert [k for k, _, _ in w[:9]] == ["range"] * 9 and all(f % B == 0 and rows == B for _, f, rows in w[:9])
        assert [f // B for _, f, _ in w[:9]] == [4, 0, 1, 2, 3, 4, 0, 1, 2]                # the first and the third call wrap
        assert all(rows == B for _, _, rows in w[:12]) and any(f % B for k, f, _ in w[9:12] if k == "step")
        assert all(f + rows <= N for _, f, rows in dc.walk(B, n, True))
        # the short tail: two announced steps on consecutive parities, the second call wraps; then a shorter host batch
        assert dc.walk(B, n, True)[:12] == w[:12] and dc.walk(B, n, True)[-dc.TAIL_STEPS:] == w[-dc.TAIL_STEPS:]
        assert all(rows == B for _, _, rows in dc.walk(B, n, True)[:-dc.TAIL_STEPS])
        (k12, f12, b), (k13, f13, b13), (k14, f14, b2) = w[12:]
        assert (k12, k13, k14) == ("range", "range", "host") and b == b13 and f13 == 0 and f12 == (N // b - 1) * b
        if n > 1:
            assert b < n and 0 in dc.shard_sizes(b, n)                                     # replicas without rows ...
            had = [r for r in range(n) if dc.shard_sizes(B, n)[r] and not dc.shard_sizes(b, n)[r]]
            assert had, (i, B, n, b)                                                       # ... which had rows two steps earlier
        if n > 2:
            assert [r for r in range(n) if dc.shard_sizes(b, n)[r] and not dc.shard_sizes(b2, n)[r]], (i, b, b2)
    assert all(2 <= _n(s) <= 3 for s in dc.LONG_CASES) and 7 in dc.LONG_CASES


_ORACLE_END = {}


def _oracle_end(i, oracle_mod):
    """Weights and momentum of the fp64 C oracle after the case's walk on whole batches."""
    if i not in _ORACLE_END:
        B = _B(i)
        X, Y = dc.case_data(i)
        ref, _ = dc.case_oracle(oracle_mod, i)
        for _, first, rows in dc.walk(B, _n(i))[:-dc.TAIL_STEPS]:
            ref.gradient_step(X[first:first + rows], Y[first:first + rows], cc.STEP, cc.MOMENTUM)
        _ORACLE_END[i] = (ref.get_weights(), ref.get_momentum())
    return _ORACLE_END[i]


def _dp_trajectory(i, oracle_mod, wrong):
    """fp64: the case's walk with the gradient formed the data-parallel way (wrong = None: correctly).  Returns the largest
    deviation of weights and momentum from the C oracle stepping on the whole batch, in units of the f32 budget."""
    dims, B, inner, out_kind, last, n, _ = dc.dp_case(i)
    X, Y = dc.case_data(i)
    wr, vr = _oracle_end(i, oracle_mod)
    w0 = dc.case_oracle(oracle_mod, i)[1]
    w, v = w0.copy(), np.zeros_like(w0)
    pidx = dc.padded_index(dims)
    npad = dc.n_pad(dims)
    live = [int(((pidx >= a) & (pidx < b)).sum()) for a, b in (dc.owner_range(npad, n, r) for r in range(n))]
    owner = max(range(n), key=lambda r: (live[r], r))                                     # the owner that holds the most weights
    lo, hi = dc.owner_range(npad, n, owner)
    in_slice = (pidx >= lo) & (pidx < hi)
    sums = []
    steps = dc.walk(B, n)[:-dc.TAIL_STEPS]                                                 # (the steps the oracle budgets apply to)
    for _, first, rows in steps:
        Ws = np_oracle.split(w, dims)
        sizes = dc.shard_sizes(rows, n)
        last_with_rows = max(r for r in range(n) if sizes[r])
        parts = []
        for r in range(n):
            a, b = dc.shard(rows, r, n)
            parts.append(np_oracle.gradient(Ws, X[first + a:first + b], Y[first + a:first + b], inner, out_kind, last) if b > a
                         else np.zeros_like(w))
        g = parts[0].copy()
        for p in parts[1:]:
            g += p
        sums.append(g.copy())
        if wrong == "drop_last":
            g = g - parts[last_with_rows]
        elif wrong == "mean_of_means":
            g = rows * sum(parts[r] / sizes[r] for r in range(n) if sizes[r]) / sum(1 for k in sizes if k)
        elif wrong == "slice_partial":
            g[in_slice] = parts[owner][in_slice]
        elif wrong == "slice_stale":
            g[in_slice] = sums[-3][in_slice] if len(sums) >= 3 else 0.0
        adj = cc.STEP * g / rows + cc.MOMENTUM * v
        w, v = w - adj, adj
    budget = W_ATOL * len(steps)
    return max(np.abs(w - wr).max(), np.abs(v - vr).max()) / budget


def test_what_the_f32_budget_catches_of_a_wrong_data_parallel_step(oracle_mod):
    """The counts of the module docstring.  Asserted: the correct sharded sum is the oracle's step (so the budget is spent on
    f32 arithmetic alone), and every wrong trajectory leaves the budget wherever it differs from the right one."""
    multi = [i for i in CASES if _n(i) > 1]
    for i in CASES:
        assert _dp_trajectory(i, oracle_mod, None) <= 1e-9, i
    counts = {}
    for wrong in ("drop_last", "mean_of_means", "slice_partial", "slice_stale"):
        used = {i: _dp_trajectory(i, oracle_mod, wrong) for i in multi}
        counts[wrong] = sum(1 for u in used.values() if u > 1.0)
        print("dp-wrong %-14s outside the budget in %d of %d cases; smallest %.3g, largest %.3g of the budget; inside: %s"
              % (wrong, counts[wrong], len(multi), min(used.values()), max(used.values()),
                 [dc.CASE_IDS[i] for i, u in used.items() if u <= 1.0]))
        if wrong == "mean_of_means":                                                     # (equal shards: the rule is the right one)
            assert all((u > 1.0) == (len(set(k for k in dc.shard_sizes(_B(i), _n(i)) if k)) > 1) for i, u in used.items()), used
        else:                                                                            # (a floor, far below what was measured)
            assert counts[wrong] >= len(multi) // 2, used
            if wrong == "slice_stale":                                                    # (a later drift of the draw or the walk shows here)
                assert [dc.CASE_IDS[i] for i, u in used.items() if u <= 1.0] == ["s12"], used


def test_a_batch_of_a_few_rows_is_outside_the_oracle_budget(oracle_mod):
    """Why the oracle budgets of the GPU sweep stop before the short tail (fp64, no GPU).  On the oracle's own trajectory of
    s21 (985-199-7-97-115-21, ReLU) the last tail step has 3 rows, and one hidden unit's pre-activation lies within 1e-4 of
    the scale sum |a||w| of its dot product, one step after a unit within 1e-6 of it: f32 arithmetic along another
    summation order may take the ReLU derivative on the other side of zero.  Taking it there for that ONE unit moves a
    weight by step * dG / rows, more than the whole walk's budget -- an error of the comparison, not of the step.  On a
    whole batch of the same net the same flip is divided by 21 rows and 0.0125."""
    i = 21
    dims, B, inner, out_kind, last, n, _ = dc.dp_case(i)
    assert inner == 3 and out_kind == cc.OUT_SOFTMAX_CE
    X, Y = dc.case_data(i)
    w = dc.case_oracle(oracle_mod, i)[1]
    v = np.zeros_like(w)
    steps = dc.walk(B, n)
    closest = []
    for s, (_, first, rows) in enumerate(steps):
        Ws = np_oracle.split(w, dims)
        Z, out = np_oracle.forward(Ws, X[first:first + rows], inner, out_kind, last)
        rel = [(np.abs(Z[l]) / (np.abs(np_oracle.act(inner, Z[l - 1])) @ np.abs(Ws[l - 1]))) for l in range(1, len(dims) - 1)]
        closest.append(min(r.min() for r in rel))
        if s == len(steps) - 1:
            l0 = int(np.argmin([r.min() for r in rel])) + 1
            b0, j0 = np.unravel_index(np.argmin(rel[l0 - 1]), rel[l0 - 1].shape)
            g = {}
            for flip in (False, True):
                D, G = out - Y[first:first + rows], []
                for l in range(len(dims) - 2, -1, -1):
                    G.append(np_oracle.act(inner, Z[l]).T @ D)
                    if l >= 1:
                        P = np_oracle.act_prime(inner, Z[l]).copy()
                        if flip and l == l0:
                            P[b0, j0] = 1.0 - P[b0, j0]
                        D = (D @ Ws[l].T) * P
                g[flip] = np.concatenate([x.ravel() for x in G[::-1]])
            assert np.array_equal(g[False], np_oracle.gradient(Ws, X[first:first + rows], Y[first:first + rows], inner, out_kind, last))
            moved = cc.STEP * np.abs(g[True] - g[False]).max() / rows
        w, v = np_oracle.gradient_step(w, v, dims, X[first:first + rows], Y[first:first + rows], cc.STEP, cc.MOMENTUM, inner, out_kind, last)
    budget = W_ATOL * len(steps)
    print("dp-tail s21: closest pre-activation per tail step %s of its scale; one flipped derivative at the last step (%d rows) moves a weight by %.3g = %.1f budgets of %d steps"
          % (", ".join("%.2g" % c for c in closest[-dc.TAIL_STEPS:]), steps[-1][2], moved, moved / budget, len(steps)))
    assert steps[-1][2] <= 3 and closest[-2] < 1e-6 and closest[-1] < 1e-4
    assert moved > 10 * budget
