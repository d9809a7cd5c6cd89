"""The drawn call sequences of tests/sequence_cases.py are the sequences tests/test_call_sequences_gpu.py is for, and its budgets
can tell a bookkeeping mistake from rounding -- conditions on the draw, no measurement of the product:

1. every lone sequence contains every planted hazard H1 .. H10 (H3 with each of its eleven followers, H6 by host batch, by range
   and by index, H7 with a sampler refill inside a batch), uses the whole vocabulary, and reaches 3 and 5 training steps at op
   boundaries (the bf16 budgets exist for those counts only);
2. at every label check at least 90 % of the rows are safe by the margins of the GPU test (1e-3 on logits, 1e-4 on General
   outputs), computed from the oracle alone;
3. for every sequence and every fault F1 .. F8 whose hazard it contains, the model with that fault lies at least two budgets from
   the correct model at the FIRST check behind the hazard -- a checkpoint, or a get_weights / get_momentum in front of it, whatever
   it shows (F8: at the first propagate behind the replacement);
4. the f32 summation-order bound that grouped validation curves are held to against the lone nets tells a validation pass on weights
   one step old.
The group sequences: every planted pair, every call form, and members 0, a middle one and the last stepped alone.

The second draw (tests/sequence_cases2.py: the calls merged since the first) leaves the first as it was -- a digest of every old op
list, computed on the commit before the second draw existed, is pinned here -- and meets the same conditions for its own hazards
H11 .. H19, its faults F9 .. F17 and its group pairs; signed perturbations leave at most adversarial_cases.UNDECIDED_CAP of the
elements undecided at every op that is compared on the decided ones."""
import numpy as np
import pytest

from tests import adversarial_cases as ac
from tests import sequence_cases as sq
from tests import sequence_cases2 as s2

VOCABULARY = {"step_host", "step_range", "step_indexed", "train_range", "train_sampled", "train_observed", "compute_gradient_range",
              "apply_update", "hint", "propagate", "loss", "argmax", "loss_range", "argmax_range", "count_hits", "evaluate", "confusion",
              "labels", "weight_gradient", "get_weights", "get_momentum", "save", "set_weights", "set_momentum", "load", "upload",
              "specialize", "forget", "advance_time", "timing", "synchronize", "sample", "refused"}
HAZARDS = ["H1", "H2"] + ["H3:" + f for f in sq.H3_FOLLOWERS] + ["H4", "H5", "H6:step_host", "H6:step_range", "H6:step_indexed",
                                                                  "H7", "H8", "H9", "H10"]


@pytest.fixture(scope="module")
def modelled(oracle_mod):
    """the correct model's run of every lone sequence, made once"""
    out = {}
    for i in range(sq.N_LONE):
        case = sq.lone_case(i)
        out[i] = (case,) + sq.run_model(oracle_mod, case)
    return out


@pytest.mark.parametrize("i", range(sq.N_LONE))
def test_every_sequence_contains_every_hazard(i):
    case = sq.lone_case(i)
    ops = case["ops"]
    assert ops == sq.lone_case(i)["ops"], "the draw is not a function of its seed"
    found = sq.hazards(ops)
    missing = [h for h in HAZARDS if h not in found]
    assert not missing, (case["id"], missing)
    # H3's followers are spread over the sequence: they lie in at least 9 different planted blocks (three ride in H6's block)
    starts = sq.draw_ops(case["draw_seed"], with_starts=True)[1]
    block_of = lambda j: sum(1 for s0 in starts if s0 <= j)
    assert len({block_of(found["H3:" + f][0]) for f in sq.H3_FOLLOWERS}) >= 9
    refills = sq.sampler_refills(ops)
    assert refills >= 1, case["id"]
    names = {name for name, _ in ops}
    assert names == VOCABULARY, (case["id"], VOCABULARY ^ names)
    assert {kw["kind"] for name, kw in ops if name == "refused"} == {"batch", "step", "rows", "validation"}
    sizes = {kw["n"] for name, kw in ops if name in ("step_host", "step_range")}
    assert len(sizes & set(sq.BATCHES)) >= 7 and 17 in sizes and sizes & {33, 40} and sizes & {1, 3}, sizes
    below = [kw["n"] <= sq.MAX_BATCH for name, kw in ops if name in sq.EVALS]
    assert any(below) and not all(below)
    V = [kw["V"] for name, kw in ops if name == "train_observed"]
    assert min(V) < sq.MAX_BATCH < max(V)
    uploads = [sq.rows_of(kw["which"]) for name, kw in ops if name == "upload"]
    assert any(n in sq.REUPLOAD_ROWS for n in uploads) and len(uploads) >= 2
    assert any(a[0] in sq.REPLACING and b[0] == "propagate" for a, b in zip(ops, ops[1:]))   # where the bf16 shadow is looked at
    print("sequence %s: %d ops, hazards at %s, %d refills inside a batch"
          % (case["id"], len(ops), " ".join("%s@%d" % (h, found[h][0]) for h in HAZARDS), refills))


@pytest.mark.parametrize("i", range(sq.N_LONE))
def test_safe_rows_and_step_counts(modelled, i):
    case, results, events, _ = modelled[i]
    steps = [r["steps"] for r in results]
    assert 3 in steps and 5 in steps, "no op boundary at 3 and 5 steps"
    assert all(np.isfinite(r[k]).all() for r in results for k in ("W", "V") if k in r), "the oracle has no finite answer"
    shares = [r["safe"].mean() for r in results if "safe" in r]              # (a check of fewer than 10 rows: every row safe)
    assert shares and min(shares) >= sq.SAFE_SHARE, (case["id"], min(shares))
    print("sequence %s: %d steps, least share of safe rows at a label check %.3f (%d checks)" % (case["id"], steps[-1], min(shares), len(shares)))


def test_the_budgets_tell_every_fault(oracle_mod, modelled):
    least = {}
    for i in range(sq.N_LONE):
        case, results, events, snaps = modelled[i]
        for fault in sq.FAULTS:
            f = sq.fault_factor(oracle_mod, case, fault, results, snaps)
            applies = (fault == "F8") == (case["dtype"] == "bf16")
            assert f is not None or not applies, "sequence %s does not contain the hazard of %s" % (case["id"], fault)
            if f is None:
                continue
            assert f >= 2.0, "sequence %s: %s stays within %.2f budgets" % (case["id"], fault, f)
            least[fault] = min(least.get(fault, np.inf), f)
    assert set(least) == set(sq.FAULTS)
    print("least distance of a faulty model, in budgets: " + "  ".join("%s %.3g" % (k, least[k]) for k in sq.FAULTS))


@pytest.mark.parametrize("i", range(sq.N_GROUP))
def test_every_group_sequence_contains_every_pair(i):
    case = sq.group_case(i)
    ops, K = case["ops"], case["K"]
    assert ops == sq.group_case(i)["ops"]
    found = sq.group_pairs(ops)
    assert sorted(found) == sorted(sq.PAIRS), (case["id"], found)
    assert {name for name, _ in ops} == set(sq.GROUP_OPS)
    assert {kw["mode"] for name, kw in ops if name == "g_train_sampled"} == {"shared", "each", "sizes"}
    alone = [(kw["k"], kw["op"][0]) for name, kw in ops if name == "member"]
    assert {k for k, _ in alone} == {0, K // 2, K - 1}
    assert {o for _, o in alone} >= {"set_weights", "load", "propagate", "evaluate", "refused", "save"} and {o for _, o in alone} & {"step_range", "step_host"}
    assert any(kw["op"][1]["n"] > sq.MAX_BATCH for name, kw in ops if name == "member" and kw["op"][0] == "evaluate")
    assert max(case["steps"]) <= sq.cc.STEP and len(set(case["steps"])) == K and len(set(case["momenta"])) == K
    for k in range(K):                                        # a lone net has a call for every op that touches member k
        lone = sq.member_case(case, k)["ops"]
        assert all((op is None) == (o[0] == "g_ensemble" or (o[0] == "member" and (o[1]["k"] != k or o[1]["op"][0] == "refused")))
                   for op, o in zip(lone, ops))
    print("group sequence %s: %d ops, pairs at %s" % (case["id"], len(ops), " ".join("%s@%d" % (p, found[p][0]) for p in sq.PAIRS)))


# (the K = 16 shape is off the grouped path: member after member, bit for bit the lone nets)
@pytest.mark.parametrize("i", [i for i in range(sq.N_GROUP) if sq.GROUPS[i // sq.SEEDS_PER_NET][0] != "g-f32-off-path-k16"])
def test_the_order_bound_tells_a_stale_validation(oracle_mod, i):
    """Grouped validation curves and loss sums are held to sequence_cases.order_bound against the lone nets (another f32 summation
    order).  A validation pass that read weights ONE STEP OLD -- the least a stale buffer can be wrong by -- returns the curve's
    previous value: every two neighbouring values of member 0's and the last member's curves lie at least two bounds apart."""
    case = sq.group_case(i)
    least = np.inf
    for k in (0, case["K"] - 1):
        mc = sq.member_case(case, k)
        m = sq.Model(oracle_mod, mc)
        for j, op in enumerate(mc["ops"]):
            if op is None:
                continue
            r = m.apply(j, op)
            if op[0] == "train_observed":
                V, val = op[1]["V"], r["val"]
                for a, b in zip(val, val[1:]):
                    least = min(least, abs(a - b) / (sq.order_bound(b * V, V) / V))
    assert least >= 2.0, (case["id"], least)
    print("group sequence %s: a validation one step stale lies at least %.3g order bounds off" % (case["id"], least))


# ---- the second draw --------------------------------------------------------------------------------------------------------------
LONE_DIGESTS = ["75c25ffe76fc97f7", "1b74b24719e56a4b", "7ee6a3d6e54af42c", "71def35c08832125", "23fce53c224e0013", "e448bd9756f0ae0f",
                "98356e2da66b174f", "d516100048e5815a", "df365d0aac5d890b", "90ebba3b37e61bf6", "985acede3aa467d9", "29a77b8e10a2d071",
                "cfd3840f50e76156", "e1acc72e5d333c42", "8ae559c11c47c48a", "36265f7dff6701e4", "efbb4b42b58b9fde", "0fbba0c5e0ed61cc",
                "f5d65805a9dd688e", "3152e1949265befe", "f1a2c6dc035e5794", "f044fb46072ae170", "675cf809943ee2cb", "a3f9028a63b2b1ef"]
GROUP_DIGESTS = ["f5112c4edf315ca4", "c1a45f3b0fd4d66b", "01decdd94c74a2d4", "feed75540b9644f7", "f4a70e6d821fe214", "ddffffbb33682803",
                 "5d77387f9962d512", "f773cbd97dd03975", "feeeb08080439338", "dfe8e482e9d40503", "37611419cac34cd9", "aad6526d9c6defac"]


def test_the_first_draw_is_what_it_was():
    """DATA_SEEDS and FAULT_FACTORS_FOUND were found on these op lists: sha256 of repr(ops), first 16 hex digits"""
    assert [s2.digest(sq.lone_case(i)["ops"]) for i in range(sq.N_LONE)] == LONE_DIGESTS
    assert [s2.digest(sq.group_case(i)["ops"]) for i in range(sq.N_GROUP)] == GROUP_DIGESTS
    assert [sq.lone_case(i)["seed"] for i in range(sq.N_LONE)] == [sq.DATA_SEEDS.get(i, 9100 + i) for i in range(sq.N_LONE)]


@pytest.fixture(scope="module")
def modelled2(oracle_mod):
    """the correct Model2's run of every sequence of the second draw, made once"""
    out = {}
    for i in range(s2.N_LONE):
        case = s2.lone_case(i)
        out[i] = (case,) + s2.run_model(oracle_mod, case)
    return out


@pytest.mark.parametrize("i", range(s2.N_LONE))
def test_every_sequence_of_the_second_draw_contains_every_hazard(i):
    case = s2.lone_case(i)
    ops, fgsm = case["ops"], s2.fgsm_ok(case["inner"])
    assert ops == s2.lone_case(i)["ops"], "the draw is not a function of its seed"
    found = s2.hazards2(ops)
    wanted = s2.HAZARDS_ALL + (s2.HAZARDS_FGSM if fgsm else [])
    missing = [h for h in wanted if h not in found]
    assert not missing, (case["id"], missing)
    names = {name for name, _ in ops}
    perturbing = {"fgsm_range", "evaluate_fgsm", "train_fgsm"}
    assert names >= set(s2.NEW_OPS) - (set() if fgsm else perturbing), (case["id"], set(s2.NEW_OPS) - names)
    assert fgsm or not names & perturbing
    refused = {kw["kind"] for name, kw in ops if name == "refused2"}
    assert refused == set(s2.REFUSALS) - ({"fgsm"} if fgsm else set())
    if not fgsm:                                                # the three perturbing calls are each refused
        assert {kw["call"] for name, kw in ops if name == "refused2" and kw["kind"] == "fgsm"} == perturbing
    else:
        assert {kw["signed"] for name, kw in ops if name == "fgsm_range"} == {False, True}
        assert {kw["held"] for name, kw in ops if name in ("fgsm_range", "evaluate_fgsm")} == {False, True}
        iters = [kw["iters"] for name, kw in ops if name == "train_fgsm"]
        assert min(iters) <= 5 and max(iters) >= 17 and all(kw["B"] in (15, 17) for name, kw in ops if name == "train_fgsm")
    assert {kw["size"] for name, kw in ops if name == "upload_held_out"} >= {57, 101}
    assert {kw["teacher"] for name, kw in ops if name == "distill"} == {"self", "other", "group"}
    assert {kw["keep"] for name, kw in ops if name == "distill"} <= set(s2.KEEPS)
    ev = [kw for name, kw in ops if name == "evaluate_set"]
    assert {kw["held"] for kw in ev} == {False, True} and {kw["kind"] for kw in ev} == {"evaluate", "confusion", "labels"}
    assert any(kw["n"] > sq.MAX_BATCH for kw in ev) and any(kw["n"] <= sq.MAX_BATCH for kw in ev)
    loops = [kw for name, kw in ops if name == "train_held_out"]
    assert {kw["rule"] for kw in loops} == {"loss", "hits"} and any(17 <= kw["iters"] <= 20 for kw in loops)
    assert min(kw["held_rows"] for kw in loops) < sq.MAX_BATCH < max(kw["held_rows"] for kw in loops)
    assert {kw["every"] for kw in loops} & {3, 7} and 1 in {kw["every"] for kw in loops}
    teacher = [kw["op"][0] for name, kw in ops if name == "teacher"]
    assert {"hint", "step_range", "step_host", "loss_range", "get_weights"} <= set(teacher)
    print("sequence %s: %d ops, hazards at %s" % (case["id"], len(ops), " ".join("%s@%d" % (h, found[h][0]) for h in wanted)))


def test_the_second_draw_covers_every_choice():
    """what one sequence need not hold, the eighteen together do"""
    ops = [op for i in range(s2.N_LONE) for op in s2.lone_case(i)["ops"]]
    assert {kw["every"] for name, kw in ops if name == "train_held_out"} == {1, 3, 7}
    assert {kw["size"] for name, kw in ops if name == "upload_held_out"} == set(s2.HELD_SIZES)
    assert {kw["keep"] for name, kw in ops if name == "distill"} == set(s2.KEEPS)
    assert {(kw["teacher"], kw["keep"]) for name, kw in ops if name == "distill"} >= {(t, 0.0) for t in ("self", "other", "group")}
    assert len({s2.lone_case(i)["net"] for i in range(s2.N_LONE)}) == 9 and s2.N_LONE == 18


@pytest.mark.parametrize("i", range(s2.N_LONE))
def test_safe_rows_and_undecided_shares_of_the_second_draw(modelled2, i):
    case, results, _ = modelled2[i]
    steps = [r["steps"] for r in results]
    assert 3 in steps and 5 in steps, "no op boundary at 3 and 5 steps"
    assert all(np.isfinite(r[k]).all() for r in results for k in ("W", "V") if k in r), "the oracle has no finite answer"
    shares = [r["safe"].mean() for r in results if "safe" in r]
    assert shares and min(shares) >= sq.SAFE_SHARE, (case["id"], min(shares))
    undecided = [1.0 - r["decided"].mean() for r in results if "decided" in r]
    assert bool(undecided) == s2.fgsm_ok(case["inner"])
    assert max(undecided or [0.0]) <= ac.UNDECIDED_CAP, (case["id"], max(undecided))
    print("sequence %s: %d steps, least share of safe rows %.3f (%d checks), largest undecided share %.4f (%d signed ops)"
          % (case["id"], steps[-1], min(shares), len(shares), max(undecided or [0.0]), len(undecided)))


def test_the_budgets_tell_every_fault_of_the_second_draw(oracle_mod, modelled2):
    """two budgets or more at the first check behind the hazard, but for the pairs of sequence_cases2.TWIN_ONLY (reasons there): any
    distance shows in the bitwise comparison with the twin that the device test makes, and must be there"""
    least, twin_only = {}, {}
    for i in range(s2.N_LONE):
        case, results, snaps = modelled2[i]
        for fault in s2.FAULTS:
            f = s2.fault_factor(oracle_mod, case, fault, results, snaps)
            applies = fault != "F12" or s2.fgsm_ok(case["inner"])          # (F12 needs a perturbing call)
            assert (f is not None) == applies, "sequence %s and the hazard of %s" % (case["id"], fault)
            if f is None:
                continue
            d = twin_only if (case["net"], fault) in s2.TWIN_ONLY else least
            assert f >= (2.0 if d is least else 1e-3), "sequence %s: %s stays within %.3g budgets" % (case["id"], fault, f)
            d[fault] = min(d.get(fault, np.inf), f)
    assert set(least) == set(s2.FAULTS)
    print("least distance of a faulty model, in budgets: " + "  ".join("%s %.3g" % (k, least[k]) for k in s2.FAULTS))
    print("... and where the twin alone resolves it: " + "  ".join("%s %.3g" % (k, v) for k, v in twin_only.items()))
    for k in s2.FAULTS:                                          # the table beside FAULT_FACTORS_FOUND is what this run finds
        assert abs(least[k] / s2.FAULT_FACTORS_FOUND2[k] - 1.0) < 0.01, (k, least[k], s2.FAULT_FACTORS_FOUND2.get(k))


@pytest.mark.parametrize("i", range(s2.N_GROUP))
def test_every_group_sequence_of_the_second_draw_contains_every_pair(i):
    case = s2.group_case(i)
    ops, K = case["ops"], case["K"]
    assert ops == s2.group_case(i)["ops"]
    found = s2.group_pairs(ops)
    assert sorted(found) == sorted(s2.PAIRS2), (case["id"], found)
    assert {name for name, _ in ops} == set(s2.GROUP_OPS2)
    assert {kw["op"][0] for name, kw in ops if name == "member"} == set(s2.MEMBER_READS)
    assert {kw["k"] for name, kw in ops if name == "member"} <= {0, K // 2, K - 1}
    loops = [kw for name, kw in ops if name == "g_train_held_out"]
    assert any(isinstance(kw["B"], list) for kw in loops) and any(17 <= kw["iters"] <= 20 for kw in loops)
    assert any(kw["held"] and kw["n"] > sq.MAX_BATCH for name, kw in ops if name == "g_evaluate_set")
    for k in range(K):
        lone = s2.member_case(case, k)["ops"]
        assert all((op is None) == (o[0] == "g_ensemble_set" or (o[0] == "member" and o[1]["k"] != k)) for op, o in zip(lone, ops))
    print("group sequence %s: %d ops, pairs at %s" % (case["id"], len(ops), " ".join("%s@%d" % (p, found[p][0]) for p in s2.PAIRS2)))
