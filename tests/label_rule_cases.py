"""Fixtures of the label-rule tests (tests/test_label_rule_cpu.py pins them and shows that the fault models below move labels,
hit counts and confusion matrices on them; tests/test_label_rule_gpu.py runs them through every label-writing head on the
device).  The reference's label is one scan (MT:166-168, MT:191-193)

    actual = 0
    for i: if out[i] >= out[actual]: actual = i

so an exact tie goes to the HIGHEST index, a NaN at an index > 0 is never selected, and a NaN at index 0 is sticky (with softmax
any NaN logit makes every probability NaN: label 0).  The rest of the suite compares labels only where the oracle's top-2 margin
is safe; here EVERY row is either tied exactly or led by a margin of thousands of budgets, and every label is compared.
No GPU code: numpy and tests/np_oracle.py.

EXACT TIES.  The last layer holds groups of IDENTICAL columns (GROUPS_*): identical weights give bit-identical logits in f32,
bf16 and fp64.  The truth is computed on ONE representative column per group (`reps`) and expanded (`colmap`); a full matrix
product is not used -- BLAS does not give duplicate columns equal bits at 300 and 1100 outputs.

WHICH GROUP WINS is set per row by selector units, built like the chain units of tests/saturation_cases.py: input column s and
hidden unit s of every layer, s = 0 .. G, chained by one positive weight, every other weight into and out of them 0; ON / OFF
inputs and the chain weight per activation are saturation_cases.CHAIN.  The last-layer row of selector g < G holds +c in group
g's columns only; the row of selector G ("down") holds -d in EVERY column.  With kappa the fp64 oracle's selector activation,
c = (LEAD + spread) / (kappa_on - kappa_off), spread being the widest row of the logits WITHOUT the selector rows: the group
on top leads every other distinct column by LEAD = 12 in the logit (60 where the last activation is leaky ReLU, whose negative
side keeps a hundredth of it).  d = 4 c; where the last activation saturates (sigmoid, tanh) d is instead chosen so that the
top pre-activation lies near 6 (the down unit's OFF state carries it: those fixtures take leaky ReLU inside, OFF = 0.5), and
there are no down rows -- their outputs would all round to the same f32 value.

ROW REGIMES.  Row i with i % 5 == 3 is a NaN row (one NaN in the last input column; the rest of it is a group row): every
output of it is NaN, the label is 0 (a ReLU LAST activation returns 0 for NaN, as the reference's does: there every output of
the row is 0 and the label n-1).  The other rows cycle group 0 .. G-1 on top / down (down ON and the next group ON: that
group on top, every logit below 0 -- the rows a padding column's 0 would win; with a ReLU last activation every output is
exactly 0, label n-1) / all-tie (an input row of zeros, only where f(0) = 0: every logit exactly 0, label n-1).  Every 4-row
block holds at least three regimes, every 16-row group a NaN row, every NaN row's block a label that is not 0.

EXPECTED CLASSES.  One-hot.  Over the rows with group g on top, in row order: hit, hit, miss, .. -- a hit expects the group's
highest index, a miss its lowest (per group more hits than misses, not as many: a fault that sends a group's ties to its LOWEST
index turns its hits into misses and its misses into hits, and with equal numbers of both the hit count would not move).  NaN rows alternate class 0 / n-1,
all-tie rows n-1 / 0.

COLUMN-NaN VARIANTS (`variant(name)`: flat weights with one last-layer weight, in the row of the last hidden unit, set to NaN
-- that column is NaN on every row).  Element-wise nets: "hi" the HIGHEST member of a tie group without column 0 (rows with
that group on top give the next lower member), "col0" (every row 0), "single" a singleton column (no label moves).  Softmax
nets: "nan", the same column as "hi" (every row 0).

THE FAULT MODELS (head_labels): numpy models of the heads' lane geometries
  quad ..... 4 lanes, lane q holds columns 4q .. 4q+3; butterfly xor 1, 2          (tail_kernel, rowblock_body's label arm)
  row16 .... 16 lanes, lane c0 holds c0, c0+16, ..; xor 1, xor 2, half-mirror, mirror  (middle4_kernel: row tail, register
             head, general head)
  reg64 .... 64 lanes, lane holds 4*lane + 256*i + j; butterfly xor 32 .. 1         (output_layer_kernel's register arm)
  scan64 ... 64 lanes, lane holds lane + 64*i; butterfly xor 32 .. 1                (its three-pass and element-wise arms)
  serial ... one thread scans every column                                          (group_forward_kernel's full head,
             group_combine_kernel's ensemble scan)
each with the step policy right / keep own (L1) / always take (L2) / lower index (L3) on equal values, a lane-local `>` (L4),
the padding columns' exact 0 in the scan (L5), the NaN flag shared by a 4-row block (L6), the softmax NaN rule on an
element-wise head (L7), the reverse (L8), a NaN at index 0 not sticky (L9), the ensemble scan with `>` (L10).

Where a fault cannot occur or cannot show (faults_for() leaves it out):
  fault   geometry / fixture                          why
  L1-L3   serial                                      no cross-lane step
  L2      quad                                        lane 0, which writes the label, holds the lowest columns and meets at each of the two
                                                      steps a partner whose columns are all higher: taking on equality IS the right rule there
  L4      row16 with <= 16 outputs, scan64 <= 64      a lane holds one column
  L5      16 outputs                                  no padding column
  L5      sigmoid last activation                     every output is > 0: a 0 never wins (tanh: the all-tie rows' exact 0s lose to it)
  L5      serial ensemble scan                        the mean probabilities are > 0
  L7, L9  softmax heads                               any NaN gives 0 by the softmax rule itself
  L6, L7, L9  ReLU last activation                    relu(NaN) = 0 in the reference (`z > 0 ? z : 0`) and in the library: no NaN reaches
                                                      the scan -- a NaN row's outputs are all 0 (label n-1), a NaN column is a column of zeros
  L8      element-wise heads                          it IS their rule
  L10     "started from 0" (best = 0, max = 0.0f)     mean probabilities are > 0 and a NaN row gives 0 either way: no label can
                                                      move; only the `>` form is asserted
"""
import numpy as np

from tests import np_oracle
from tests import saturation_cases as sc

LEAKY, SIGMOID, TANH, RELU, IDENT = sc.LEAKY, sc.SIGMOID, sc.TANH, sc.RELU, sc.IDENT
SCE, GENERAL = sc.SCE, sc.GENERAL
F32, BF16 = sc.F32, sc.BF16
BUDGET = sc.BUDGET
LEAD, LEAD_LEAKY_LAST, TOP_SATURATING = 12.0, 60.0, 6.0
MIN_LEAD_BUDGETS = 100.0
R_NAN, R_DOWN, R_TIE = -1, -2, -3            # row regimes; 0 .. G-1: that group on top

GROUPS_10 = [(0, 9), (7, 8), (2, 5), (3, 4, 6)]
GROUPS_16 = [(0, 15), (7, 8), (3, 12), (5, 6, 10)]
# 17 outputs: identical columns are an equivalence, so pairs (0,16) and (15,16) are ONE group -- column 0, its +16 successor
# (the same lane of the general head) and lane 15
GROUPS_17 = [(0, 15, 16), (3, 12), (7, 8), (5, 13)]
GROUPS_40 = [(3, 35), (19, 20), (7, 39), (0, 16, 32)]
GROUPS_300 = [(5, 261), (255, 256), (0, 299), (3, 4), (100, 101, 290)]
GROUPS_1100 = [(10, 74), (63, 64), (0, 1099), (1087, 1088), (100, 612, 1000)]

#         name       dims                    out      inner    last     rows  groups
_TABLE = [
    ("T3",     [20, 12, 10],            SCE,     LEAKY,   IDENT,   21, GROUPS_10),
    ("T4",     [20, 12, 8, 10],         SCE,     TANH,    IDENT,   37, GROUPS_10),
    ("T4s",    [20, 12, 8, 10],         SCE,     SIGMOID, IDENT,   21, GROUPS_10),    # no all-tie rows: f(0) = 0.5
    ("T16",    [20, 12, 8, 16],         SCE,     LEAKY,   IDENT,   37, GROUPS_16),    # 16 outputs: no padding column
    ("T132",   [20, 132, 10],           SCE,     LEAKY,   IDENT,   21, GROUPS_10),    # middle4's register head
    ("T17",    [20, 12, 17],            SCE,     TANH,    IDENT,   37, GROUPS_17),    # middle4's general head
    ("T40",    [20, 12, 9, 8, 7, 40],   SCE,     IDENT,   IDENT,   21, GROUPS_40),
    ("T300",   [40, 24, 300],           SCE,     LEAKY,   IDENT,   21, GROUPS_300),   # the output kernel's register arm, two chunks
    ("T1100",  [40, 24, 1100],          SCE,     LEAKY,   IDENT,   21, GROUPS_1100),  # its three-pass arm
    ("TS",     [784, 100, 50, 10],      SCE,     LEAKY,   IDENT,   29, GROUPS_10),    # the prebuilt static instances
    ("GS",     [784, 100, 50, 10],      GENERAL, TANH,    IDENT,   29, GROUPS_10),
    ("G_ident", [20, 12, 8, 10],        GENERAL, TANH,    IDENT,   21, GROUPS_10),
    ("G_leaky", [20, 12, 8, 10],        GENERAL, IDENT,   LEAKY,   21, GROUPS_10),
    ("G_relu", [20, 12, 8, 10],         GENERAL, TANH,    RELU,    21, GROUPS_10),
    ("G_sigm", [20, 12, 8, 10],         GENERAL, LEAKY,   SIGMOID, 21, GROUPS_10),
    ("G_tanh", [20, 12, 8, 10],         GENERAL, LEAKY,   TANH,    21, GROUPS_10),
    ("G17_ident", [20, 12, 17],         GENERAL, TANH,    IDENT,   21, GROUPS_17),
    ("G17_leaky", [20, 12, 17],         GENERAL, IDENT,   LEAKY,   21, GROUPS_17),
    ("G17_relu", [20, 12, 17],          GENERAL, TANH,    RELU,    21, GROUPS_17),
    ("G17_sigm", [20, 12, 17],          GENERAL, LEAKY,   SIGMOID, 21, GROUPS_17),
    ("G17_tanh", [20, 12, 17],          GENERAL, LEAKY,   TANH,    21, GROUPS_17),
]
NAMES = [r[0] for r in _TABLE]
SOFTMAX_NAMES = [r[0] for r in _TABLE if r[2] == SCE]
GENERAL_NAMES = [r[0] for r in _TABLE if r[2] == GENERAL]
GROUP_NAMES = ["T4", "T16"]            # the NetGroup cases
GROUP_SEEDS = (1, 2, 3)


def label_scan(row):
    """MT:166-168, literally."""
    actual = 0
    for i in range(len(row)):
        if row[i] >= row[actual]:
            actual = i
    return actual


def hits_of(labels, Y):
    return int((np.asarray(labels) == expected_class(Y)).sum())


def expected_class(Y):
    """The last index whose expected value is 1 (MT:186-188)."""
    return np.array([int(np.flatnonzero(r == 1)[-1]) for r in Y])


def confusion_of(labels, Y):
    """[e, p] counts; a label outside 0 .. n-1 (what a fault model may give) is counted in an extra last column."""
    n = Y.shape[1]
    conf = np.zeros((n, n + 1), dtype=np.int64)
    for e, p in zip(expected_class(Y), np.asarray(labels)):
        conf[e, p if 0 <= p < n else n] += 1
    return conf


class Fixture:
    """One net, its weights (f32-exact, flat `w` and per layer `Ws`), rows X (f32-exact, with NaNs), expected rows Y, the regime
    of every row (`regime`) and the group on top of it (`top`, -1 on all-tie rows)."""

    def __init__(self, oracle_mod, name, dims, out_kind, inner, last, rows, groups, seed=1, like=None):
        self.name, self.dims, self.out_kind, self.inner, self.last, self.rows = name, dims, out_kind, inner, last, rows
        self.groups = [tuple(g) for g in groups]
        d0, n, Lm, G = dims[0], dims[-1], len(dims) - 1, len(groups)
        nsel = G + 1
        assert min(dims[:-1]) > nsel
        assert len({c for g in groups for c in g}) == sum(len(g) for g in groups) and all(list(g) == sorted(g) for g in groups)
        self.group_of = np.full(n, -1)
        for gi, g in enumerate(groups):
            self.group_of[list(g)] = gi
        # one representative per set of identical columns, in column order
        self.reps = np.array([j for j in range(n) if self.group_of[j] < 0 or groups[self.group_of[j]][0] == j])
        rep_of = np.array([j if self.group_of[j] < 0 else groups[self.group_of[j]][0] for j in range(n)])
        self.colmap = np.searchsorted(self.reps, rep_of)
        saturating = out_kind == GENERAL and last in (SIGMOID, TANH)
        self.has_tie = inner != SIGMOID
        self.has_down = not saturating
        on, off, wc = sc.CHAIN[inner]

        Ws = sc._scaled_draw(oracle_mod, dims, out_kind, inner, last, seed)
        for l in range(Lm - 1):
            for u in range(nsel):
                Ws[l][u, :] = 0.0
                Ws[l][:, u] = 0.0
                Ws[l][u, u] = wc
        Ws[Lm - 1][:nsel, :] = 0.0
        for g in groups:
            for j in g[1:]:
                Ws[Lm - 1][:, j] = Ws[Lm - 1][:, g[0]]

        if like is None:
            X, _ = sc._candidates(7000 + 10 * len(dims) + n, rows, d0)
            cycle = list(range(G)) + ([R_DOWN] if self.has_down else []) + ([R_TIE] if self.has_tie else [])
            self.regime, self.top = np.zeros(rows, dtype=int), np.zeros(rows, dtype=int)
            k = t = 0
            for i in range(rows):
                if i % 5 == 3:
                    self.regime[i], self.top[i] = R_NAN, t % G
                    t += 1
                else:
                    r = cycle[k % len(cycle)]
                    k += 1
                    self.regime[i] = r
                    if r == R_TIE:
                        self.top[i] = -1
                    elif r == R_DOWN:
                        self.top[i] = t % G
                        t += 1
                    else:
                        self.top[i] = r
            X[:, :nsel] = off
            for i in range(rows):
                if self.regime[i] == R_TIE:
                    X[i, :] = 0.0
                    continue
                X[i, self.top[i]] = on
                if self.regime[i] == R_DOWN:
                    X[i, G] = on
                if self.regime[i] == R_NAN:
                    X[i, d0 - 1] = np.nan
            # expected classes
            want, seen, a, b = np.zeros(rows, dtype=int), [0] * G, 0, 0
            for i in range(rows):
                if self.regime[i] == R_NAN:
                    want[i] = 0 if a % 2 == 0 else n - 1
                    a += 1
                elif self.regime[i] == R_TIE:
                    want[i] = n - 1 if b % 2 == 0 else 0
                    b += 1
                else:
                    g = groups[self.top[i]]
                    want[i] = g[-1] if seen[self.top[i]] % 3 != 2 else g[0]
                    seen[self.top[i]] += 1
            self.Y = np.eye(n)[want]
        else:
            X, self.Y, self.regime, self.top = like.X.copy(), like.Y, like.regime, like.top
        self.X = X

        # c and d from the oracle's own selector activations and the widest row of the logits without the selector rows
        live = ~np.isin(self.regime, (R_NAN, R_TIE))
        Z, _ = np_oracle.forward(Ws, X[live], inner, out_kind, last)
        K = np_oracle.act(inner, Z[Lm - 1])[:, :nsel]
        first = int(np.flatnonzero(self.regime[live] == 0)[0])
        k_on, k_off = float(K[first, 0]), float(K[first, 1])
        assert np.allclose(K[:, :G][self.top[live][:, None] == np.arange(G)[None, :]], k_on, rtol=1e-12)
        spread = float((Z[-1].max(axis=1) - Z[-1].min(axis=1)).max())
        lead = LEAD_LEAKY_LAST if (out_kind == GENERAL and last == LEAKY) else LEAD
        self.c = float(np.float32((lead + spread) / (k_on - k_off)))
        if saturating:
            assert k_off > 0
            self.d = float(np.float32((self.c * k_on - TOP_SATURATING) / k_off))
        else:
            self.d = float(np.float32(4.0 * self.c))
        for gi, g in enumerate(groups):
            Ws[Lm - 1][gi, list(g)] = self.c
        Ws[Lm - 1][G, :] = -self.d
        self.Ws = [sc.f32(W) for W in Ws]
        self.w = np.concatenate([W.ravel() for W in self.Ws])
        self.k_on, self.k_off, self.spread = k_on, k_off, spread

        # the column-NaN variants: {name: column}
        g_hi = next(g for g in groups if 0 not in g)
        single = int(np.flatnonzero(self.group_of < 0)[0])
        assert single != 0 and g_hi[-1] != n - 1
        self.nan_cols = {"nan": g_hi[-1]} if out_kind == SCE else {"hi": g_hi[-1], "col0": 0, "single": single}
        self.hi_group = groups.index(g_hi)
        self._truths = {}

    def __repr__(self):
        return self.name

    def variant(self, name):
        """The flat weights with the variant's last-layer weight (row of the last hidden unit) set to NaN."""
        W = [x.copy() for x in self.Ws]
        W[-1][self.dims[-2] - 1, self.nan_cols[name]] = np.nan
        return np.concatenate([x.ravel() for x in W])

    def truth(self, dtype, variant=None):
        key = (dtype, variant)
        if key not in self._truths:
            self._truths[key] = Truth(self, dtype, variant)
        return self._truths[key]


class Truth:
    """Z: logits / last pre-activations; out: probabilities / outputs (NaN rows all NaN); key: what a head scans and what the
    lead is measured in (softmax: the logits, which order as the probabilities do; else the outputs); label; hits; conf."""

    def __init__(self, fx, dtype, variant=None, jitter=None):
        Wr = fx.Ws[:-1] + [np.ascontiguousarray(fx.Ws[-1][:, fx.reps])]
        a = (fx.inner, fx.out_kind, fx.last)
        with np.errstate(all="ignore"):
            if dtype == BF16:
                Z = np_oracle.forward_bf16(Wr, fx.X, *a, jitter=jitter)[0]
            else:
                Z = np_oracle.forward(Wr, fx.X, *a)[0]
            self.Z = Z[-1][:, fx.colmap].copy()
            if variant is not None:
                self.Z[:, fx.nan_cols[variant]] = np.nan     # an activation (0 included) times NaN
            if fx.out_kind == SCE:
                nan_row = np.isnan(self.Z).any(axis=1)
                zs = np.where(nan_row[:, None], 0.0, self.Z)
                e = np.exp(zs - zs.max(axis=1, keepdims=True))
                self.out = e / e.sum(axis=1, keepdims=True)
                self.out[nan_row] = np.nan                    # one NaN logit: every probability NaN (SCE:368)
                self.key = self.Z
            else:
                self.out = np_oracle.act(fx.last, self.Z)
                self.key = self.out
        self.label = np.array([label_scan(r) for r in self.out])
        self.hits = hits_of(self.label, fx.Y)
        self.conf = confusion_of(self.label, fx.Y)[:, :-1]


_fixtures = {}


def fixture(oracle_mod, name, seed=1):
    """The fixture (seed 1), or the net of Random(seed) with the same groups and selectors on the same rows: a further member
    of a net group."""
    if (name, seed) not in _fixtures:
        row = next(r for r in _TABLE if r[0] == name)
        _fixtures[(name, seed)] = Fixture(oracle_mod, *row) if seed == 1 else Fixture(oracle_mod, *row, seed=seed, like=fixture(oracle_mod, name))
    return _fixtures[(name, seed)]


def ensemble_truth(members, dtype, nan_member=None):
    """(mean, label, hits, conf) of the member-order f32 mean of the members' probabilities; nan_member: that member with its
    "nan" variant."""
    outs = [m.truth(dtype, "nan" if k == nan_member else None).out for k, m in enumerate(members)]
    with np.errstate(all="ignore"):
        acc = outs[0].astype(np.float32)
        for o in outs[1:]:
            acc = acc + o.astype(np.float32)
        mean = (acc / np.float32(len(outs))).astype(np.float64)
    label = np.array([label_scan(r) for r in mean])
    Y = members[0].Y
    return mean, label, hits_of(label, Y), confusion_of(label, Y)[:, :-1]


def lead_in_budgets(fx, t, dtype):
    """The smallest lead of the winning group over every other distinct column, over the rows with a group on top, in units of
    the dtype's output budget; rows whose outputs are all equal (all-tie rows, a ReLU head's down rows) and NaN rows have none."""
    worst = np.inf
    for i in range(fx.rows):
        r = t.key[i]
        if np.isnan(r).any() or (r == r[0]).all():
            continue
        g = fx.groups[fx.top[i]]
        others = np.delete(r, list(g))
        assert (r[list(g)] == r[g[0]]).all()
        worst = min(worst, (r[g[0]] - others.max()) / BUDGET[dtype]["p"])
    return worst


# ---- numpy models of the heads: the right one and the faults the device tests must be able to see ------------------
GEOMETRIES = ("quad", "row16", "reg64", "scan64", "serial")
STEPS = {"quad": (1, 2), "row16": (1, 2, 7, 15), "reg64": (32, 16, 8, 4, 2, 1), "scan64": (32, 16, 8, 4, 2, 1), "serial": ()}
LANES = {"quad": 4, "row16": 16, "reg64": 64, "scan64": 64, "serial": 1}


def lane_columns(geom, n_cols):
    """Per lane the columns it scans, ascending."""
    if geom == "quad":
        assert n_cols <= 16
        return [[c for c in range(4 * q, 4 * q + 4) if c < n_cols] for q in range(4)]
    if geom == "row16":
        return [list(range(c0, n_cols, 16)) for c0 in range(16)]
    if geom == "reg64":
        return [[4 * l + 256 * i + j for i in range(4) for j in range(4) if 4 * l + 256 * i + j < n_cols] for l in range(64)]
    if geom == "scan64":
        return [list(range(l, n_cols, 64)) for l in range(64)]
    return [list(range(n_cols))]


def head_labels(out, geom, softmax, step="right", local_ge=True, pad=False, block_nan=False, nan_rule=None, sticky0=True):
    """The labels a head of geometry `geom` gives on the f32 rows `out`.  step: what a cross-lane step does on EQUAL values --
    "right" (the higher index), "own" (L1), "take" (L2), "lower" (L3).  local_ge=False: the lane-local scan with `>` (L4).
    pad: the padding columns up to a multiple of 16, exact zeros, join the scan (L5).  block_nan: the NaN flag is shared by
    the rows of a 4-row block (L6).  nan_rule "softmax" / "elementwise": the other head's rule (L7, L8).  sticky0=False: no
    NaN flag at all on an element-wise head (L9)."""
    out = np.asarray(out, dtype=np.float32)
    rows, n = out.shape
    width = (n + 15) // 16 * 16 if pad else n
    cols = lane_columns(geom, width)
    lanes = np.arange(LANES[geom])
    rule = nan_rule or ("softmax" if softmax else "elementwise")
    labels, flags = np.zeros(rows, dtype=int), np.zeros(rows, dtype=bool)
    for r in range(rows):
        row = np.r_[out[r], np.zeros(width - n, dtype=np.float32)]
        mx = np.full(len(lanes), -np.inf, dtype=np.float32)
        best = np.full(len(lanes), -1)
        for l, cl in enumerate(cols):
            for c in cl:
                v = row[c]
                if (v >= mx[l]) if local_ge else (v > mx[l]):      # (a NaN compares false: never taken)
                    mx[l], best[l] = v, c
        for x in STEPS[geom]:
            ov, ob = mx[lanes ^ x], best[lanes ^ x]
            eq = ov == mx
            take = (ov > mx) | (eq & {"right": ob > best, "own": np.zeros_like(eq), "take": np.ones_like(eq), "lower": ob < best}[step])
            mx, best = np.where(take, ov, mx), np.where(take, ob, best)
        labels[r] = best[0]
        flags[r] = np.isnan(out[r]).any() if rule == "softmax" else (sticky0 and bool(np.isnan(out[r, 0])))
    if block_nan:
        for b in range(0, rows, 4):
            flags[b:b + 4] = flags[b:b + 4].any()
    labels[flags] = 0
    return labels


FAULTS = {
    "L1": dict(step="own"), "L2": dict(step="take"), "L3": dict(step="lower"), "L4": dict(local_ge=False), "L5": dict(pad=True),
    "L6": dict(block_nan=True), "L7": dict(nan_rule="softmax"), "L8": dict(nan_rule="elementwise"), "L9": dict(sticky0=False),
    "L10": dict(local_ge=False),
}
# the variant of the fixture on which a NaN-rule fault shows (None: the fixture itself)
FAULT_VARIANTS = {"L7": ("hi", "single"), "L8": ("nan",), "L9": ("col0",)}


def geometries_for(fx):
    """The lane geometries the fixture's routes reach (tests/test_label_rule_gpu.py)."""
    n = fx.dims[-1]
    if fx.out_kind == GENERAL:
        return ("quad", "row16", "scan64") if n <= 16 else ("row16", "scan64")
    if n <= 16:
        return ("quad", "row16", "reg64", "serial") if fx.name in GROUP_NAMES else ("quad", "row16", "reg64")
    if n <= 64:
        return ("row16",)
    return ("reg64",) if n <= 1024 else ("scan64",)


def faults_for(fx, geom):
    """The faults that can occur in `geom` and can show on `fx` (the module docstring's table says why the others cannot)."""
    n, softmax = fx.dims[-1], fx.out_kind == SCE
    out = []
    if geom != "serial":
        out += ["L1", "L3"] if geom == "quad" else ["L1", "L2", "L3"]
    if max(len(c) for c in lane_columns(geom, n)) > 1:
        out.append("L4")
    if n % 16 != 0 and not (fx.out_kind == GENERAL and fx.last == SIGMOID):
        out.append("L5")
    if softmax:
        out += ["L6", "L8"]
    elif fx.last != RELU:
        out += ["L6", "L7", "L9"]
    return out
