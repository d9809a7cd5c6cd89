"""Pins what tests/tile_merge_cases.py must hold for tests/test_tile_merge_cases_gpu.py to mean anything (no GPU): the draw, the
geometries the shapes plant (counted from the host checker's per-entry report of make_merged_tile_map), the batch sizes and call
forms the schedules run on them, make_merged_tile_map's invariants over a sweep of shapes, and -- from the fp64 oracle -- that the
fixtures can see a fault and that the reference alone stays well inside the budget the device is held to."""
import numpy as np
import pytest

from tests import chain_cases as cc
from tests import np_oracle
from tests import tile_merge_cases as tc

CUS = 32             # CUs per XCD of the MI355X
DRAWN = [[204, 170, 67, 4], [92, 149, 101, 96, 10], [68, 116, 15], [216, 122, 9], [303, 124, 12], [177, 289, 7, 2], [139, 182, 29, 9], [84, 138, 46, 5]]
# (first row, rows) of the announced schedule's 14 steps
ANNOUNCED_WALK = [(0, 16), (97, 144), (194, 16), (480, 120), (388, 128), (184, 300), (81, 100), (334, 256), (176, 1), (408, 136), (28, 130), (121, 128),
                  (579, 16), (347, 144)]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    out = tc.build_checker(tmp_path_factory.mktemp("tile_merge_cases"))
    if out is None:
        pytest.skip("no hipcc")
    return out


@pytest.fixture(scope="module")
def reports(checker):
    return {c.name: tc.entries(checker, c.dims, CUS) for c in tc.CASES}


def padded(b):
    return tc.pad(b)


def features(oracle_mod, case):
    """What the case's schedule runs: names from the list in test_every_schedule_feature_on_every_geometry."""
    out = set()
    batches = tc.call_batches(oracle_mod, case, case.schedule)
    sizes = [len(idx) for call in batches for idx in call]
    for b in sizes:
        for name, hit in (("B=1", b == 1), ("B=16", b == 16), ("ragged B<112", b < 112 and b % 16), ("B in 113..127", 113 <= b <= 127),
                          ("B=128", b == 128), ("B in 129..143", 129 <= b <= 143), ("B=144", b == 144), ("B=256", b == 256),
                          ("ragged B in 257..303", 257 <= b <= 303 and b % 16)):
            if hit:
                out.add(name)
    for call, idxs in zip(case.schedule, batches):
        if call[0] == "range" and call[3] > 1:
            firsts = [int(i[0]) for i in idxs]
            if any(b < a for a, b in zip(firsts, firsts[1:])) and any(int(i[-1]) == case.rows - 1 for i in idxs):
                out.add("a walk that wraps, one batch ending at the last row")
        if call[0] == "sampled" and min(len(i) for i in idxs) < call[2]:
            out.add("sampled, a shortened batch, B < 128" if call[2] < 128 else "sampled, a shortened batch, B >= 128")
    if case.recut is not None:
        out.add("a second cut")
    steps = [c for c in case.schedule if c[0] == "step"]
    right = [(a[2], b[2]) for a, b in zip(steps, steps[1:]) if a[3] == (b[1], b[2])]
    wrong = [a for a, b in zip(steps, steps[1:]) if a[3] is not None and a[3] != (b[1], b[2])]
    if any(padded(a) < 128 <= padded(b) and padded(a) != padded(b) for a, b in right) and any(padded(b) < 128 <= padded(a) for a, b in right) and wrong:
        out.add("announced, padded sizes differ both ways across 128, one announcement wrong")
    return out


FEATURES = ["B=1", "B=16", "ragged B<112", "B in 113..127", "B=128", "B in 129..143", "B=144", "B=256", "ragged B in 257..303",
            "a walk that wraps, one batch ending at the last row", "a second cut", "sampled, a shortened batch, B < 128",
            "sampled, a shortened batch, B >= 128", "announced, padded sizes differ both ways across 128, one announcement wrong"]


def geometry(report):
    """The geometric classes of a shape's merged map."""
    ents, summary = report
    out = set()
    if not summary["usable"]:
        return out
    out.add("usable")
    for e in ents:
        if e.kind == tc.GROUP:
            out.add("a %d-row group" % e.height)
        if e.kind == tc.PAIR and e.height < tc.TM:
            out.add("a pair on a partial tile row")
    return out


def test_the_draw_and_the_schedules_are_pinned():
    assert [tc.drawn_dims(i) for i in range(tc.N_DRAWN)] == DRAWN
    assert [c.dims for c in tc.CASES] == [c.dims for c in tc._cases()]
    for i, d in enumerate(DRAWN):
        assert 1 <= d[0] < 400 and 3 <= len(d) <= 6 and all(1 <= w <= 384 for w in d[1:-1]) and d[-2] <= 128 and 2 <= d[-1] < 17
    assert len(tc.CASES) == 4 * len(tc.CARRIERS) + (len(tc.PLANTED) - len(tc.CARRIERS)) + tc.N_DRAWN + 4 and len(set(tc.IDS)) == len(tc.IDS)
    for c in tc.CASES:
        assert tc.n_steps(c.schedule) <= tc.MAX_STEPS and (c.recut is None or tc.n_steps(c.recut) == tc.n_steps(c.schedule))
        for call in c.schedule + (c.recut or []):
            B = call[2]
            assert 1 <= B <= c.max_batch
            if call[0] != "sampled":
                assert 0 <= call[1] and call[1] + B <= c.rows
            if call[0] == "step" and call[3] is not None:
                assert 0 <= call[3][0] and 1 <= call[3][1] <= c.max_batch and sum(call[3]) <= c.rows
    assert tc.sizes_schedule()[1] == [("range", 599, 1, 2), ("range", 576, 16, 2), ("range", 500, 100, 2), ("range", 480, 120, 2), ("range", 384, 128, 2),
                                      ("range", 0, 136, 1), ("range", 432, 144, 1), ("range", 256, 256, 2), ("range", 300, 300, 1)]
    assert [(c[1], c[2]) for c in tc.announced_schedule()[1]] == ANNOUNCED_WALK
    assert [s for s, c in enumerate(tc.announced_schedule()[1][:-1]) if c[3] != ANNOUNCED_WALK[s + 1]] == [3, 9]
    assert tc.sampled_schedule(100) == (351, [("sampled", 5, 100), ("sampled", 4, 100)], [("sampled", 2, 100), ("sampled", 7, 100)])
    assert tc.headline_schedule() == (600, [("range", 0, 128, 6), ("range", 360, 120, 6)], None)
    kinds = [c.kind for c in tc.CASES if c.dims[0] >= 784]
    assert kinds == ["headline"] * 4 and all(c.dims[0] < 784 for c in tc.CASES if c.kind != "headline")
    # both net classes, every inner activation, every last activation
    assert {c.out_kind for c in tc.CASES} == {tc.OUT_SOFTMAX_CE, tc.OUT_ACT_LOSS} and {c.inner for c in tc.CASES} == {0, 1, 2, 3}
    assert {c.last for c in tc.CASES if c.out_kind == tc.OUT_ACT_LOSS} == set(cc.LAST_ACTS)


def test_schedules_repeat_their_steps_under_the_second_cut(oracle_mod):
    """recut runs the same rows in the same order, cut into calls differently."""
    for c in tc.CASES:
        if c.recut is None:
            continue
        a = [i for call in tc.call_batches(oracle_mod, c, c.schedule) for i in call]
        b = [i for call in tc.call_batches(oracle_mod, c, c.recut) for i in call]
        assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b)), c.name
        assert [x[:3] for x in c.recut] != [x[:3] for x in c.schedule] or c.kind == "announced"


def test_every_case_keeps_the_row_block_path_and_all_but_one_are_usable(reports):
    for c in tc.CASES:
        _, s = reports[c.name]
        assert s["rb_ok"] == 1 and tc.rb_ok(c.dims), c.name
        assert s["usable"] == (c.dims != tc.NOT_USABLE), c.name
        assert s["owned"] == s["expected"] and s["multiply_owned"] == s["out_of_layer"] == s["odd_pairs"] == s["mismatches"] == 0, c.name
    assert not tc.rb_ok([784, 304, 128, 16])      # (why 784-304-96-16 stands in for it: tile_merge_cases.py)
    s = reports["800-300-100-10-headline"][1]
    assert s["max_xcd"] == 33 and s["usable"] == 0
    for name in ("784-300-100-10-headline", "784-304-96-16-headline"):
        assert reports[name][1]["max_xcd"] == 32 and reports[name][1]["grid"] == 256, name
    assert reports["784-304-96-16-headline"][1]["singles"] == 2     # layer 1 in pairs only; the two singles are layer 2's


def test_the_planted_geometries_occur(reports):
    """Counted from the per-entry report, over the usable cases: what the issue's list plants."""
    def of(dims):
        return next(reports[c.name] for c in tc.CASES if c.dims == dims)
    usable = [reports[c.name] for c in tc.CASES if reports[c.name][1]["usable"]]
    ents = [e for r in usable for e in r[0]]
    # layer 0 with no whole tile at all, at both group heights
    no_whole = [r for r in usable if r[1]["whole"] == 0]
    assert {e.height for r in no_whole for e in r[0] if e.kind == tc.GROUP} == {16, 32}
    assert all(r[1]["plan_regular"] == 0 and r[1]["regular"] == 0 for r in no_whole)        # no head: every slot by lookup
    # a partial row whose rows are mostly padding: one live row of 16, 26 of 32
    assert any(e.kind == tc.GROUP and (e.height, e.live_rows) == (16, 1) for e in ents)
    assert any(e.kind == tc.GROUP and (e.height, e.live_rows) == (32, 26) for e in ents)
    assert any(e.kind == tc.GROUP and e.height == 16 and e.live_rows == 1 for e in of([1, 17, 10])[0]) and of([1, 17, 10])[1]["whole"] == 0
    assert any(e.kind == tc.GROUP and e.height == 16 and e.live_rows == 1 for e in of([65, 100, 70, 10])[0])
    # every size of a group, the short last ones among them; a layer 0 that is one column wide
    assert {e.cols for e in ents if e.kind == tc.GROUP and e.height == 16} == {1, 2, 3, 4}
    assert {e.cols for e in ents if e.kind == tc.GROUP and e.height == 32} == {1, 2}
    assert [(e.kind, e.cols) for e in of([16, 16, 2])[0]] == [(tc.GROUP, 1), (tc.SINGLE, 1)]
    assert [e.cols for e in of([12, 300, 100, 10])[0] if e.kind == tc.GROUP] == [4, 4, 4, 4, 3]
    assert [e.cols for e in of([20, 300, 100, 10])[0] if e.kind == tc.GROUP] == [2] * 9 + [1]
    assert [e.cols for e in of([32, 33, 10])[0] if e.kind == tc.GROUP] == [2, 1]
    assert [e.cols for e in of([80, 96, 16])[0] if e.kind == tc.GROUP] == [4, 2]
    assert [e.cols for e in of([80, 80, 10])[0] if e.kind == tc.GROUP] == [4, 1]
    assert [e.cols for e in of([96, 64, 10])[0] if e.kind == tc.GROUP] == [2, 2]
    assert [e.cols for e in of([90, 112, 80, 5])[0] if e.kind == tc.GROUP] == [2, 2, 2, 1]
    # a 48-row only row counts as whole: regular slots, no group (the <= 32 boundary)
    r = of([33, 48, 10])
    assert r[1]["groups"] == 0 and r[1]["whole"] == 3 and r[1]["regular"] == 3
    # later layers: partial tile rows of 16, 32 and 48 rows; pairs and single columns on such rows; six layers
    later = [e for e in ents if e.layer > 0 and e.height < tc.TM]
    assert {e.height for e in later} == {16, 32, 48}
    assert {e.height for e in later if e.kind == tc.PAIR} == {16, 32, 48} and {e.height for e in later if e.kind == tc.SINGLE} == {16, 32, 48}
    assert any(e.live_rows < e.height for e in later if e.kind == tc.PAIR)                 # (a pair's m0 + er < L.M guard cuts rows off)
    r = of([129, 16, 16, 16, 16, 2])
    assert len(r[0]) == 7 and max(e.layer for e in r[0]) == 4 and all(e.cols == 1 for e in r[0])
    assert {len(c.dims) for c in tc.CASES} == {3, 4, 5, 6}


def test_every_schedule_feature_on_every_geometry(oracle_mod, reports):
    """Every batch size class and call form occurs on a usable shape, on one with a 16-row group, on one with a 32-row group and on
    one with a pair on a partial tile row of a later layer."""
    have = {}
    for c in tc.CASES:
        if c.kind == "headline":
            continue                                        # (the 784-wide shapes add 128 and 120 in train_range; not counted)
        for f in features(oracle_mod, c):
            have.setdefault(f, set()).update(geometry(reports[c.name]))
    for f in FEATURES:
        assert have.get(f, set()) >= {"usable", "a 16-row group", "a 32-row group", "a pair on a partial tile row"}, (f, have.get(f))
    for c in tc.CASES:
        if c.kind == "headline":
            assert features(oracle_mod, c) >= {"B=128", "B in 113..127", "a walk that wraps, one batch ending at the last row"}, c.name


def test_the_sweep_reports_no_violation(checker):
    """Every padded first width 16..1024 x second width 16..384 x three tails x 4, 8 and 32 CUs per XCD: each tile has one owner, no
    unit leaves its tile row or layer, pairs start at even columns, usable == (max_xcd <= cus), make_tile_head has no mismatch."""
    import subprocess
    r = subprocess.run([checker, "sweep"], check=True, capture_output=True, text=True, timeout=120)
    f = r.stdout.split()
    m = dict(zip(f[0::2], map(int, f[1::2])))
    assert m["maps"] == 3 * 64 * 24 * 3 and m["violations"] == 0


@pytest.mark.parametrize("case", tc.CASES, ids=tc.IDS)
def test_the_fixture_can_see_a_fault_and_the_reference_is_inside_the_budget(oracle_mod, case):
    """From the fp64 oracle.  (1) At the end of the schedule every weight and every momentum element has moved: no tile's update
    can go missing unseen.  (2) In every step every hidden unit of layer 1 has a non-zero gradient into a weight of layer 0's
    partial tile row (its last tile row where it has no partial one): a wrong or stale slab piece changes the step after it.
    (3) The schedule restated in float32 numpy ends within a quarter of W_ATOL x steps of the oracle: the budget holds the device
    to the reference's own f32 error times four, no more."""
    d0, d1 = case.dims[0], case.dims[1]
    rows = tc.partial_row_inputs(case.dims)
    assert rows.size and rows[-1] == d0 - 1
    X, _ = tc.case_data(case)
    assert np.all(X[:, rows] > 0)                            # every batch, of one row too, feeds every weight row of the groups
    dead = []

    def observe(ref, x, y):
        g = np_oracle.gradient(np_oracle.split(ref.get_weights(), case.dims), x, y, case.inner, case.out_kind, case.last)
        g0 = g[:d0 * d1].reshape(d0, d1)[rows]
        dead.append(int(np.sum(~np.any(g0 != 0, axis=0))))
    w0, w, v = tc.trajectory(oracle_mod, case, observe)
    assert len(dead) == tc.n_steps(case.schedule) and not any(dead), dead
    assert np.isfinite(w).all() and np.all(w != w0) and np.all(v != 0), (int(np.sum(w == w0)), int(np.sum(v == 0)))
    w32, v32 = tc.trajectory_f32(oracle_mod, case)
    assert w32.dtype == np.float32 and v32.dtype == np.float32
    budget = tc.W_ATOL * tc.n_steps(case.schedule)
    dw, dv = np.abs(w32 - w).max(), np.abs(v32 - v).max()
    print("tile-merge case %s: f32 restatement dw %.3f dv %.3f of the budget %.3g" % (case.name, dw / budget, dv / budget, budget))
    assert dw <= budget / 4 and dv <= budget / 4, (dw, dv, budget)
    assert np.abs(w - w0).max() > 100 * budget              # the trajectory moves the weights far beyond the budget
