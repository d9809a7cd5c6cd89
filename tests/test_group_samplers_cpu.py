"""The fixtures of tests/test_group_samplers_gpu.py (a group call with one sampler per member) do what those tests need -- shown
with the CPU oracle's sampler alone.  A batch is shortened at a refill by a row drawn twice (NNT:149-155), per sampler, so
around a refill the members' batch sizes may differ: such an iteration is stepped member after member, every other one by the
grouped launches.  The GPU tests take their expected (grouped, member after member) counts from `predict` below, never from
typed-in numbers; the table of this module says where the sizes differ, and the test reproduces it."""
import numpy as np
import pytest

# name: (rows N, batch, iterations, sampler seeds, draws made before the call per sampler)
FIXTURES = {
    "F1": (203, 48, 13, [1, 1, 7], None),
    "F2": (40, 12, 14, [1, 2, 3], None),
    "F3": (50, 16, 12, list(range(1, 17)), None),
    "F4": (203, 48, 13, [1, 1, 7], [0, 20, 45]),
    # F1 run on into the fifth sampler chunk of the training loop (csrc/sample_ring.h: the chunks begin at iterations 0, 16, 48,
    # 112, 240), which reuses slot 0 of the loop's ring of four chunk slots; its properties are computed below, not tabulated
    "F5": (203, 48, 260, [1, 1, 7], None),
}
F5_SIZES = (48, 40, 24)  # the batch sizes F5's samplers draw with in tests/test_group_batches_gpu.py (one size per member)
RING_SLOTS = 4
# iterations (0-based) whose batch sizes differ between the members; and those with a shortened batch of ONE size for all
DIFFER = {"F1": [4, 12], "F2": [3, 6, 13], "F3": [3, 6, 9], "F4": [3, 4, 7, 8, 11, 12]}
AGREE_SHORT = {"F1": [8], "F2": [], "F3": [], "F4": []}
SIZES = {("F1", 4): (45, 45, 43), ("F1", 12): (46, 46, 45), ("F1", 8): (46, 46, 46)}
GROUPED_MIXED = {"F1": (11, 2), "F2": (11, 3), "F3": (9, 3), "F4": (7, 6)}


def batch_sizes(oracle_mod, name, iterations=None, skip=0):
    """(iterations, K) batch sizes the fixture's samplers draw, after `skip` earlier iterations of the same batch size."""
    N, batch, iters, seeds, advance = FIXTURES[name]
    iterations = iters if iterations is None else iterations
    out = np.empty((iterations, len(seeds)), dtype=np.int64)
    for k, seed in enumerate(seeds):
        s = oracle_mod.Sampler(N, seed=seed)
        if advance and advance[k]:
            s.sample(advance[k])
        for _ in range(skip):
            s.sample(batch)
        for i in range(iterations):
            out[i, k] = len(s.sample(batch))
    return out


def predict(oracle_mod, name, iterations=None, skip=0):
    """(grouped, member_after_member) of one call on a group with grouped launches, and the list of mixed iterations."""
    sizes = batch_sizes(oracle_mod, name, iterations, skip)
    mixed = [i for i in range(sizes.shape[0]) if len(set(sizes[i])) > 1]
    return (sizes.shape[0] - len(mixed), len(mixed)), mixed


def chunk_starts(iterations, cap=256):
    """First iterations of the training loop's sampler chunks: 16, 32, 64, .. iterations doubling up to `cap`, then `cap` each."""
    starts, begin, size = [], 0, min(16, cap)
    while begin < iterations:
        starts.append(begin)
        begin, size = begin + size, min(cap, size * 2)
    return starts


def chunk_of(starts, i):
    return max(c for c, s in enumerate(starts) if s <= i)


def test_f5_crosses_four_chunk_boundaries_and_the_rings_wrap(oracle_mod):
    """Every chunk of F5 holds an iteration whose batch sizes differ between the members, the first iteration of chunk 1 is one
    (its predecessor meets a mixed successor across a chunk boundary), and chunk 4 reuses the ring slot of chunk 0."""
    N, batch, iters, seeds, _ = FIXTURES["F5"]
    starts = chunk_starts(iters)
    assert starts == [0, 16, 48, 112, 240] and len(starts) == RING_SLOTS + 1  # (the schedule of csrc/sample_ring.h, cap 256)
    sizes = batch_sizes(oracle_mod, "F5")
    assert np.array_equal(sizes[:FIXTURES["F1"][2]], batch_sizes(oracle_mod, "F1"))  # F1 run on
    (grouped, mixed_n), mixed = predict(oracle_mod, "F5")
    per_chunk = [sum(1 for i in mixed if chunk_of(starts, i) == c) for c in range(len(starts))]
    print("F5: %d iterations whose sizes differ, per chunk %s, smallest batch %d" % (mixed_n, per_chunk, sizes.min()))
    assert all(n >= 1 for n in per_chunk)
    assert starts[1] in mixed
    assert sizes.min() >= 43
    assert grouped > 0 and grouped + mixed_n == iters


def test_f5_samplers_with_a_size_per_member_meet_a_refill_in_every_chunk(oracle_mod):
    """F5's samplers drawing F5_SIZES: every chunk contains a batch that a refill shortened for ONE member only."""
    N, _, iters, seeds, _ = FIXTURES["F5"]
    starts = chunk_starts(iters)
    sizes = np.empty((iters, len(seeds)), dtype=np.int64)
    for k, (seed, b) in enumerate(zip(seeds, F5_SIZES)):
        s = oracle_mod.Sampler(N, seed=seed)
        sizes[:, k] = [len(s.sample(b)) for _ in range(iters)]
    assert max(F5_SIZES) < N and (sizes <= np.array(F5_SIZES)).all() and sizes.min() >= 1
    short = sizes != np.array(F5_SIZES)
    one_only = [i for i in range(iters) if short[i].sum() == 1]
    per_chunk = [sum(1 for i in one_only if chunk_of(starts, i) == c) for c in range(len(starts))]
    print("F5 with sizes %s: batches shortened for one member only, per chunk %s" % (F5_SIZES, per_chunk))
    assert all(n >= 1 for n in per_chunk)


@pytest.mark.parametrize("name", sorted(DIFFER))
def test_fixture_has_the_iterations_the_gpu_tests_need(oracle_mod, name):
    N, batch, iters, seeds, _ = FIXTURES[name]
    sizes = batch_sizes(oracle_mod, name)
    assert sizes.shape == (iters, len(seeds)) and batch < N
    (grouped, mixed_n), mixed = predict(oracle_mod, name)
    assert mixed == DIFFER[name]
    assert (grouped, mixed_n) == GROUPED_MIXED[name]
    short_same = [i for i in range(iters) if len(set(sizes[i])) == 1 and sizes[i, 0] < batch]
    assert short_same == AGREE_SHORT[name]
    for i in range(iters):  # every other iteration is a full batch for every member
        if i not in mixed and i not in short_same:
            assert (sizes[i] == batch).all()
    for (fx, i), want in SIZES.items():
        if fx == name:
            assert tuple(sizes[i]) == want
    assert grouped > 0 and mixed_n > 0  # both routes are taken


def test_second_call_pattern_is_predicted_from_the_samplers_state(oracle_mod):
    """A second call continues the samplers: its pattern is the tail of one long run's."""
    N, batch, iters, seeds, _ = FIXTURES["F1"]
    both = batch_sizes(oracle_mod, "F1", iters + 6)
    assert np.array_equal(batch_sizes(oracle_mod, "F1", 6, skip=iters), both[iters:])
    (grouped, mixed_n), mixed = predict(oracle_mod, "F1", 6, skip=iters)
    assert grouped + mixed_n == 6 and mixed == [i - iters for i in range(iters, iters + 6) if len(set(both[i])) > 1]


def test_equal_seeds_draw_equal_batches_until_advanced(oracle_mod):
    """F1's samplers 0 and 1 share a seed: equal sizes in every iteration; F4 advances one of them, and they part."""
    f1, f4 = batch_sizes(oracle_mod, "F1"), batch_sizes(oracle_mod, "F4")
    assert np.array_equal(f1[:, 0], f1[:, 1])
    assert not np.array_equal(f4[:, 0], f4[:, 1])
