"""What the five sampled training entry points of a NetGroup REFUSE (csrc/group.hip: gnn_mlp_group_train_sampled, _observed,
_each, _sizes, _held_out): one table of argument defects, and of pairs of defects, with the status each returns and the text
gnn_mlp_last_error() then holds -- the literals of the library's source, a pair's those of the refusal that stands FIRST there.
After every refused call the same call with good arguments runs, the group stays bit for bit (weights, momentum, step count of
every member, the curves it returns) the twin group that made the good calls only, and every sampler draws what its twin draws:
a refused call has stepped nothing and drawn nothing.  Run on a group with grouped launches and on one without (the member-after-
member route), so that the refusals are seen in front of both."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GROUPED = [784, 300, 100, 10]
OFF_PATH = [784, 1024, 1024, 1024, 10]   # off the two-launch path: launches_per_step == 0
K, N, MAX_BATCH, HELD = 2, 300, 64, 40
BAD_ARG, UNSUPPORTED, STATE = 1, 3, 5

# the good call; a table row replaces some of its entries.  samplers: indices into the group's own two, "other" (a sampler of
# N + 1 rows), None (a null entry); the entry points with ONE sampler take samplers[0], ONE batch size batches[0].  The steps are
# small: a group makes up to 37 good calls in a row on random labels, and the 1024-wide net must stay finite through them.
GOOD = dict(group=True, samplers=(0, 1), iterations=3, batches=(32, 32), steps=(0.0001, 0.0002), momenta=(0.9, 0.8), noise=0,
            V=4, val=True, every=2, held_rows=HELD, rule=0, hits=True)

NULL_GROUP = "null group"
PER_MEMBER = "steps and momenta: one value per member, not null"
STEP = "step must be positive (SCE:301)"
NULL_SAMPLERS = "samplers is null"
NULL_BATCHES = "batches is null: one batch size per member"
NULL_SAMPLER = "null sampler"
TWICE = "the same sampler for two members: every member draws from its own"
SIZE = "sampler size differs from the dataset"
BELOW = "batchSize must be below the data size (NNT:63)"
MAX = "B exceeds max_batch given to gnn_mlp_create"
EMPTY = "batch must be non-empty"
ITER = "iterations must be positive (NNT:62)"
NOISE = "noise=true is not built on the GPU (SCE:335)"
VSIZE = "validation size outside the dataset (NNT:104)"
NULL_OUT = "null output"
EVERY = "every must be positive"
RULE = "rule: GNN_BEST_LOSS or GNN_BEST_HITS"
HELD_ROWS = "held_rows outside the held-out set"
NO_HELD = "no held-out set uploaded"

# what every entry point refuses in its first two blocks
_COMMON = [
    ("null group", dict(group=False), BAD_ARG, NULL_GROUP),
    ("null steps", dict(steps=None), BAD_ARG, PER_MEMBER),
    ("null momenta", dict(momenta=None), BAD_ARG, PER_MEMBER),
    ("a step of 0 for member 1", dict(steps=(0.0001, 0.0)), BAD_ARG, STEP),
    ("a negative step for member 0", dict(steps=(-0.0001, 0.0002)), BAD_ARG, STEP),
    ("iterations 0", dict(iterations=0), BAD_ARG, ITER),
    ("noise", dict(noise=1), UNSUPPORTED, NOISE),
    ("PAIR null group + null steps", dict(group=False, steps=None), BAD_ARG, NULL_GROUP),
    ("PAIR noise + iterations 0", dict(noise=1, iterations=0), UNSUPPORTED, NOISE),
]
_ONE_SAMPLER = [
    ("a null sampler", dict(samplers=None), BAD_ARG, NULL_SAMPLER),
    ("a sampler of another size", dict(samplers=("other",)), BAD_ARG, SIZE),
    ("batch above max_batch", dict(batches=(MAX_BATCH + 1,)), BAD_ARG, MAX),
    ("batch 0", dict(batches=(0,)), BAD_ARG, EMPTY),
    ("batch == N", dict(batches=(60,), rows=60), BAD_ARG, BELOW),
    ("PAIR null steps + a null sampler", dict(steps=None, samplers=None), BAD_ARG, PER_MEMBER),
    ("PAIR a sampler of another size + batch above max_batch", dict(samplers=("other",), batches=(MAX_BATCH + 1,)), BAD_ARG, MAX),
]
_PER_MEMBER_SAMPLERS = [
    ("null samplers", dict(samplers=None), BAD_ARG, NULL_SAMPLERS),
    ("a null sampler among K", dict(samplers=(0, None)), BAD_ARG, NULL_SAMPLER),
    ("one sampler given twice", dict(samplers=(0, 0)), BAD_ARG, TWICE),
    ("a sampler of another size for member 1", dict(samplers=(0, "other")), BAD_ARG, SIZE),
    ("a sampler of another size for member 0", dict(samplers=("other", 1)), BAD_ARG, SIZE),
    ("PAIR a null sampler among K + the other given twice", dict(samplers=(None, None)), BAD_ARG, NULL_SAMPLER),
    ("PAIR one sampler given twice + iterations 0", dict(samplers=(1, 1), iterations=0), BAD_ARG, TWICE),
    ("PAIR null momenta + null samplers", dict(momenta=None, samplers=None), BAD_ARG, PER_MEMBER),
]
_CURVE = [
    ("validation_size 0 with a curve asked for", dict(V=0), BAD_ARG, VSIZE),
    ("validation_size N + 1 with a curve asked for", dict(V=N + 1), BAD_ARG, VSIZE),
    ("PAIR iterations 0 + validation_size 0", dict(iterations=0, V=0), BAD_ARG, ITER),
]
_BATCH_ARRAY = [
    ("null batches", dict(batches=None), BAD_ARG, NULL_BATCHES),
    ("member 1's batch above max_batch", dict(batches=(32, MAX_BATCH + 1)), BAD_ARG, MAX),
    ("member 1's batch 0", dict(batches=(32, 0)), BAD_ARG, EMPTY),
    ("member 1's batch == N", dict(batches=(32, 60), rows=60), BAD_ARG, BELOW),
    ("PAIR null batches + a null sampler among K", dict(batches=None, samplers=(0, None)), BAD_ARG, NULL_BATCHES),
    ("PAIR null samplers + null batches", dict(samplers=None, batches=None), BAD_ARG, NULL_SAMPLERS),
    ("PAIR null batches + one sampler given twice", dict(batches=None, samplers=(0, 0)), BAD_ARG, NULL_BATCHES),
    ("PAIR one sampler given twice + member 1's batch above max_batch", dict(samplers=(0, 0), batches=(32, MAX_BATCH + 1)), BAD_ARG, TWICE),
]

TABLE = {
    "sampled": _COMMON + _ONE_SAMPLER,
    "observed": _COMMON + _ONE_SAMPLER + _CURVE + [
        ("null val_loss", dict(val=False), BAD_ARG, NULL_OUT),
        ("PAIR null val_loss + noise", dict(val=False, noise=1), UNSUPPORTED, NOISE),
        ("PAIR null val_loss + validation_size 0", dict(val=False, V=0), BAD_ARG, NULL_OUT),
        ("PAIR null val_loss + a sampler of another size", dict(val=False, samplers=("other",)), BAD_ARG, SIZE),
    ],
    "each": _COMMON + _PER_MEMBER_SAMPLERS + _CURVE + [
        ("batch above max_batch", dict(batches=(MAX_BATCH + 1,)), BAD_ARG, MAX),
        ("batch == N", dict(batches=(60,), rows=60), BAD_ARG, BELOW),
        ("PAIR one sampler given twice + validation_size 0", dict(samplers=(0, 0), V=0), BAD_ARG, TWICE),
        ("PAIR a sampler of another size for member 1 + validation_size 0", dict(samplers=(0, "other"), V=0), BAD_ARG, SIZE),
        ("PAIR noise + validation_size N + 1", dict(noise=1, V=N + 1), UNSUPPORTED, NOISE),
    ],
    "sizes": _COMMON + _PER_MEMBER_SAMPLERS + _CURVE + _BATCH_ARRAY + [
        ("PAIR member 1's batch above max_batch + validation_size 0", dict(batches=(32, MAX_BATCH + 1), V=0), BAD_ARG, MAX),
    ],
    "held_out": _COMMON + _PER_MEMBER_SAMPLERS + _BATCH_ARRAY + [
        ("every 0", dict(every=0), BAD_ARG, EVERY),
        ("a rule that is neither", dict(rule=2), BAD_ARG, RULE),
        ("held_rows 0", dict(held_rows=0), BAD_ARG, HELD_ROWS),
        ("held_rows above the set", dict(held_rows=HELD + 1), BAD_ARG, HELD_ROWS),
        ("no held-out set uploaded", dict(held=False), STATE, NO_HELD),
        ("null point_hits", dict(hits=False), BAD_ARG, NULL_OUT),
        ("PAIR a rule that is neither + one sampler given twice", dict(rule=2, samplers=(0, 0)), BAD_ARG, TWICE),
        ("PAIR every 0 + iterations 0", dict(every=0, iterations=0), BAD_ARG, ITER),
        ("PAIR null point_hits + a rule that is neither", dict(hits=False, rule=2), BAD_ARG, NULL_OUT),
        ("PAIR a rule that is neither + every 0", dict(rule=2, every=0), BAD_ARG, RULE),
        ("PAIR every 0 + no held-out set uploaded", dict(every=0, held=False), BAD_ARG, EVERY),
        ("PAIR held_rows 0 + member 1's batch 0", dict(held_rows=0, batches=(32, 0)), BAD_ARG, EMPTY),
    ],
}


class _Side:
    """One group with its samplers: the one that is refused, or its twin."""

    def __init__(self, gnn, dims, X, Y, held):
        self.g = gnn.NetGroup(dims, [1, 2], max_batch=MAX_BATCH)
        self.g.upload_dataset(X, Y)
        if held is not None:
            self.g.upload_held_out(*held)
        self.samplers = [gnn.Sampler(len(X), seed=k + 1) for k in range(K)]
        self.other = gnn.Sampler(len(X) + 1, seed=7)

    def call(self, entry, **defects):
        """The entry point's raw call with GOOD's arguments but for `defects`: (status, last error, what it wrote)."""
        a = dict(GOOD, **defects)
        lib, dp, i64 = self.g._lib, C.POINTER(C.c_double), C.POINTER(C.c_int64)
        pick = lambda s: None if s is None else self.other._h if s == "other" else self.samplers[s]._h
        g = self.g._h if a["group"] else None
        steps, moms = (None if v is None else (C.c_double * K)(*v) for v in (a["steps"], a["momenta"]))
        val = np.zeros((max(a["iterations"], 0), K))
        out = val.ctypes.data_as(dp) if a["val"] else None
        if entry in ("sampled", "observed"):
            s = None if a["samplers"] is None else pick(a["samplers"][0])
            if entry == "sampled":
                rc, wrote = lib.gnn_mlp_group_train_sampled(g, s, a["iterations"], a["batches"][0], steps, moms, a["noise"]), ()
            else:
                rc, wrote = lib.gnn_mlp_group_train_sampled_observed(g, s, a["iterations"], a["batches"][0], steps, moms, a["noise"], a["V"], out), (val,)
        else:
            ss = None if a["samplers"] is None else (C.c_void_p * K)(*[pick(s) for s in a["samplers"]])
            bs = None if a["batches"] is None else (C.c_int32 * K)(*(a["batches"] * K)[:K])
            if entry == "each":
                rc, wrote = lib.gnn_mlp_group_train_sampled_each(g, ss, a["iterations"], a["batches"][0], steps, moms, a["noise"], a["V"], out), (val,)
            elif entry == "sizes":
                rc, wrote = lib.gnn_mlp_group_train_sampled_sizes(g, ss, a["iterations"], bs, steps, moms, a["noise"], a["V"], out), (val,)
            else:
                P = 2  # the good call's points: behind iterations 2 and 3
                hits, loss, ens, best = np.zeros((P, K), np.int64), np.zeros((P, K)), np.zeros(P, np.int64), np.zeros(K, np.int32)
                rc = lib.gnn_mlp_group_train_sampled_held_out(g, ss, a["iterations"], bs, steps, moms, a["noise"], a["every"], a["held_rows"], a["rule"],
                                                              hits.ctypes.data_as(i64) if a["hits"] else None, loss.ctypes.data_as(dp),
                                                              ens.ctypes.data_as(i64), best.ctypes.data_as(C.POINTER(C.c_int32)), None)
                wrote = (hits, loss, ens, best)
        return rc, (lib.gnn_mlp_last_error() or b"").decode(), wrote

    def close(self):
        for x in self.samplers + [self.other, self.g]:
            x.close()


def _data(n, seed=0):
    rng = np.random.default_rng(seed)
    return rng.random((n, GROUPED[0])), np.eye(GROUPED[-1])[rng.integers(0, GROUPED[-1], n)]


def _pair(gnn, dims, rows, held):
    """The group to refuse and its twin on `rows` training rows; held False: the first has no held-out set yet."""
    X, Y = _data(rows)
    Xh, Yh = _data(HELD, seed=1)
    return _Side(gnn, dims, X, Y, (Xh, Yh) if held else None), _Side(gnn, dims, X, Y, (Xh, Yh))


@pytest.mark.parametrize("entry", list(TABLE))
@pytest.mark.parametrize("dims,launches", [(GROUPED, 2), (OFF_PATH, 0)], ids=["grouped", "member-after-member"])
def test_refusals(gnn, dims, launches, entry):
    pairs = {}  # by training rows: made when a row first needs it, then kept through the rows that follow
    for what, defects, code, text in TABLE[entry]:
        defects = dict(defects)
        rows, held = defects.pop("rows", N), defects.pop("held", True)
        if not held:
            a, b = _pair(gnn, dims, rows, False)
        else:
            if rows not in pairs:
                pairs[rows] = _pair(gnn, dims, rows, True)
            a, b = pairs[rows]
        assert a.g.launches_per_step == launches
        rc, msg, _ = a.call(entry, **defects)
        print("%-8s %-70s -> %d %r" % (entry, what, rc, msg))
        assert rc == code and text in msg, (what, rc, msg)
        if not held:  # (the good call needs the set)
            a.g.upload_held_out(*_data(HELD, seed=1))
        # the same call with good arguments runs, and leaves the group its twin's equal: nothing was stepped ...
        (rc_a, msg_a, out_a), (rc_b, _, out_b) = a.call(entry), b.call(entry)
        assert rc_a == 0 and rc_b == 0, (what, rc_a, msg_a)
        for x, y in zip(out_a, out_b):
            assert np.array_equal(x, y) and np.isfinite(x).all(), what
        for k in range(K):
            m, t = a.g.members[k], b.g.members[k]
            assert m.time == t.time, (what, k)
            assert np.array_equal(m.get_weights(), t.get_weights()), (what, k)
            assert np.array_equal(m.get_momentum(), t.get_momentum()), (what, k)
        # ... and nothing drawn, from the group's samplers or from the one it must not take
        for s, t in zip(a.samplers + [a.other], b.samplers + [b.other]):
            assert np.array_equal(s.sample(32), t.sample(32)), what
        if not held:
            a.close(); b.close()
    for a, b in pairs.values():
        a.close(); b.close()


def test_the_table_covers_what_it_is_there_for():
    rows = {e: {w: d for w, d, _, _ in TABLE[e]} for e in TABLE}
    assert set(TABLE) == {"sampled", "observed", "each", "sizes", "held_out"}
    for e, r in rows.items():
        assert len(r) == len(TABLE[e]), "a row's name twice: " + e
        assert {"null group", "null steps", "null momenta", "a step of 0 for member 1", "iterations 0", "noise"} <= set(r), e
        assert any("batch == N" in w for w in r) and any("above max_batch" in w for w in r), e
        assert any(w.startswith("PAIR") for w in r), e
    for e in ("each", "sizes", "held_out"):
        assert {"null samplers", "a null sampler among K", "one sampler given twice", "a sampler of another size for member 1"} <= set(rows[e]), e
    for e in ("observed", "each", "sizes"):
        assert {"validation_size 0 with a curve asked for", "validation_size N + 1 with a curve asked for"} <= set(rows[e]), e
    for e in ("sizes", "held_out"):
        assert "null batches" in rows[e], e
    assert "null val_loss" in rows["observed"]
    assert {"every 0", "a rule that is neither", "held_rows 0", "held_rows above the set", "no held-out set uploaded", "null point_hits"} <= set(rows["held_out"])
    # the pairs whose two refusals sit in different blocks of the source
    assert rows["observed"]["PAIR null val_loss + noise"] == dict(val=False, noise=1)
    assert rows["sizes"]["PAIR null batches + a null sampler among K"] == dict(batches=None, samplers=(0, None))
    assert rows["each"]["PAIR one sampler given twice + validation_size 0"] == dict(samplers=(0, 0), V=0)
    assert rows["held_out"]["PAIR a rule that is neither + one sampler given twice"] == dict(rule=2, samplers=(0, 0))
