"""The fixtures of tests/group_batch_cases.py contain what tests/test_group_batches_gpu.py needs -- shown with the CPU oracle's
sampler alone (as tests/test_group_samplers_cpu.py does for the calls with one batch size for all).  A group call with one batch
size per member steps EVERY iteration with the two grouped launches, member k with its own live row count; what can go wrong
there goes wrong where the members' counts part: different 16-row pads, one and two TS_KC chunks of the tile kernels, a single
row, a batch a refill shortened for one member only."""
import numpy as np
import pytest

from tests import group_batch_cases as bc


def _pad(b):
    return (b + bc.PAD - 1) // bc.PAD * bc.PAD


@pytest.mark.parametrize("name", sorted(bc.FIXTURES))
def test_table_of_shortened_batches_is_the_oracles(oracle_mod, name):
    N, batches, iters, sseeds, wseeds = bc.FIXTURES[name]
    assert len(batches) == len(sseeds) == len(wseeds) and max(batches) < N
    sizes = bc.batch_sizes(oracle_mod, name)
    assert sizes.shape == (iters, len(batches))
    assert bc.shortened(sizes, batches) == bc.SHORTENED[name]
    assert ((sizes >= 1) & (sizes <= np.array(batches))).all()


@pytest.mark.parametrize("name", sorted(bc.FIXTURES))
def test_every_fixture_has_members_of_different_nominal_sizes(name):  # 1
    assert len(set(bc.FIXTURES[name][1])) > 1


def test_some_fixture_pads_to_different_multiples_of_16():  # 2
    assert any(len({_pad(b) for b in f[1]}) > 1 for f in bc.FIXTURES.values())
    assert len({_pad(b) for b in bc.FIXTURES["RAGGED"][1]}) == 2


def test_some_fixture_has_one_and_two_chunks(oracle_mod):  # 3
    batches = bc.FIXTURES["CHUNKS"][1]
    assert min(batches) <= bc.TS_KC < max(batches)
    # ... and live: an iteration in which one member runs two chunks while another runs one, one in which a member of two chunks
    # comes down to exactly one full chunk, and to less, and the member at 128 on the guarded path (fewer than 128 rows) beside it
    sizes = bc.batch_sizes(oracle_mod, "CHUNKS")
    assert any(_pad(r.max()) > bc.TS_KC >= _pad(r.min()) for r in sizes)
    assert any(r[3] == bc.TS_KC and r[2] < bc.TS_KC for r in sizes)
    assert any(r[3] < bc.TS_KC for r in sizes) and any(r[3] == 130 for r in sizes)


def test_some_fixture_has_a_member_with_batch_1():  # 4
    assert sum(1 in f[1] for f in bc.FIXTURES.values()) >= 1


@pytest.mark.parametrize("name", sorted(bc.FIXTURES))
def test_every_fixture_has_a_refill_that_shortens_one_member_only(oracle_mod, name):  # 5
    batches = bc.FIXTURES[name][1]
    sizes = bc.batch_sizes(oracle_mod, name)
    whole = sizes == np.array(batches)
    assert any((~whole[i]).any() and whole[i].any() for i in range(sizes.shape[0]))


@pytest.mark.parametrize("name", sorted(bc.FIXTURES))
def test_a_member_changes_size_while_the_others_keep_theirs(oracle_mod, name):  # 6 (asked of one fixture; every one has it)
    """The iteration that turns `rb_next` (plan.hip) off for all: announced for member k is another size than it is stepping."""
    sizes = bc.batch_sizes(oracle_mod, name)
    changed = sizes[1:] != sizes[:-1]
    assert any(changed[i].any() and not changed[i].all() for i in range(changed.shape[0]))


def test_second_call_of_the_sweep_continues_the_samplers(oracle_mod):
    a, b = bc.SWEEP_CALLS
    assert a + b == bc.FIXTURES["SWEEP"][2]
    both = bc.batch_sizes(oracle_mod, "SWEEP")
    assert np.array_equal(bc.batch_sizes(oracle_mod, "SWEEP", b, skip=a), both[a:])
    assert bc.shortened(both[:a], bc.FIXTURES["SWEEP"][1]) and bc.shortened(both[a:], bc.FIXTURES["SWEEP"][1])  # both calls meet one
