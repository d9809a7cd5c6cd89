"""What the tests of a group's observed training loop share (NetGroup.train_sampled_observed, gnn_mlp_group_train_sampled_observed):
the drawn nets of tests/chain_cases.py in groups, the fixture of the fp64 oracle comparison, and the two tolerances.

(alpha)  Two fp64 sums of the same V non-negative f32 values in different orders differ by at most about V * 2^-53 relative --
         below 1e-12 for V <= 4 000.  A curve against another form's curve of the SAME per-row losses: |a - b| <= 1e-12 |b|.
(beta)   The project's budget for a mean loss of the 784-100-50-10 f32 net of the oracle fixture against the fp64 oracle:
         2e-4 |v| + 2e-4 (tests/test_trainer_gpu.py: test_observed_training_loops_run_on_the_device; tests/test_group_eval_gpu.py)."""
import numpy as np

from tests import chain_cases as cc

ALPHA = 1e-12

# (seed, dtype, K) of tests/chain_cases.py: the groups tests/test_group_gpu.py steps in grouped launches ...
GROUPED_CASES = [(0, 0, 16), (6, 0, 5), (10, 0, 2), (12, 0, 5), (14, 0, 16), (16, 0, 2), (17, 0, 5), (20, 0, 2),
                 (2, 1, 5), (14, 1, 2), (18, 1, 16), (22, 1, 2)]
# ... and member after member (17 first-layer K slabs; no row-block kernel), a group of one net, and a bf16 group whose route is
# read from launches_per_step
FALLBACK_CASES = [(7, 0, 2), (13, 0, 5)]
MEMBER_ROUTE_CASES = FALLBACK_CASES + [(6, 0, 1), (12, 1, 2)]
SEGMENTS = (17, 7)          # two calls; between them member 0 alone takes a step on a host batch
LONE_STEP = (0.02, 0.8)     # ... with this step size and momentum
REFILL_CASE = (12, 0, 5)    # 300 iterations in ONE call, V = 64: the curve matrix (256 rows) is summed and refilled
REFILL_ITERATIONS, REFILL_V = 300, 64


def case_hyper(K):
    """Distinct per member, all near the cases' own 0.0125 / 0.9 (as tests/test_group_gpu.py: _case_hyper)."""
    return [cc.STEP * (1 + k / 32) for k in range(K)], [cc.MOMENTUM - 0.01 * k for k in range(K)]


def id_of(case):
    return "seed%d-%s-K%d" % (case[0], "bf16" if case[1] else "f32", case[2])


def validation_rows(B):
    """V = N - 3: ragged, several 32-row tiles for most cases."""
    return cc.dataset_rows(B) - 3


def budget(v):
    return 2e-4 * np.abs(v) + 2e-4


def close_alpha(a, b):
    """(alpha), after checking that everything is finite."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.isfinite(a).all() and np.isfinite(b).all() and (np.abs(a - b) <= ALPHA * np.abs(b)).all())


# ---- the fp64 oracle on the drawn cases ---------------------------------------------------------------------------------------
def drawn_oracle_curves(oracle_mod, seed, members, segments, V, lone_step=True):
    """The curves of the case's members (a list of member indices k: seed k + 1, case_hyper's step and momentum) in the fp64
    oracle over the tests' call sequence: (sum(segments), len(members))."""
    dims, B, inner, out_kind, last = cc.chain_case(seed)
    N = cc.dataset_rows(B)
    X, Y = cc.chain_data(seed, dims, B)
    steps, moms = case_hyper(max(members) + 1)
    out = np.empty((sum(segments), len(members)))
    for j, k in enumerate(members):
        ref = oracle_mod.OracleNet(dims, out_kind=out_kind, inner_act=inner, last_act=last, seed=k + 1)
        ref.set_alloc_per_sample(0)
        ref.set_weights(ref.get_weights().astype(np.float32).astype(np.float64) * cc.W_SCALE)
        smp = oracle_mod.Sampler(N, seed=cc.SAMPLER_SEED)
        i = 0
        for s, n in enumerate(segments):
            if s and lone_step and k == 0:
                ref.gradient_step(X[B:2 * B], Y[B:2 * B], *LONE_STEP)
            for _ in range(n):
                idx = smp.sample(B)
                ref.gradient_step(X[idx], Y[idx], steps[k], moms[k])
                out[i, j] = ref.calculate_loss(X[:V], Y[:V]).mean()
                i += 1
        ref.close()
    return out


# ---- the oracle fixture: the data of test_observed_training_loops_run_on_the_device, three members -----------------------------
ORACLE_DIMS, ORACLE_N, ORACLE_B, ORACLE_ITERATIONS = [784, 100, 50, 10], 640, 32, 12
ORACLE_SEEDS = [1, 2, 3]
ORACLE_STEPS, ORACLE_MOMENTA = [0.01, 0.014, 0.018], [0.9, 0.85, 0.8]
ORACLE_V = (7, 150)


def oracle_data():
    """pixels (80 % zero), labels, and the rows as the nets see them."""
    rng = np.random.default_rng(12)
    pix = rng.integers(0, 256, (ORACLE_N, 784), dtype=np.uint8)
    pix[rng.random((ORACLE_N, 784)) < 0.8] = 0
    lab = rng.integers(0, 10, ORACLE_N, dtype=np.uint8)
    return pix, lab, pix / 255.0, np.eye(10)[lab]


_oracle_curves = {}


def oracle_curves(oracle_mod):
    """{V: (ORACLE_ITERATIONS, 3)}: validate(V) (NNT:102-113) of every member on the oracle's own trajectory, computed once."""
    if not _oracle_curves:
        _, _, X, Y = oracle_data()
        out = {V: np.empty((ORACLE_ITERATIONS, len(ORACLE_SEEDS))) for V in ORACLE_V}
        for k, seed in enumerate(ORACLE_SEEDS):
            ref = oracle_mod.OracleNet(ORACLE_DIMS, seed=seed)
            ref.set_alloc_per_sample(0)
            smp = oracle_mod.Sampler(ORACLE_N)
            for i in range(ORACLE_ITERATIONS):
                idx = smp.sample(ORACLE_B)
                ref.gradient_step(X[idx], Y[idx], ORACLE_STEPS[k], ORACLE_MOMENTA[k])
                for V in ORACLE_V:
                    out[V][i, k] = ref.calculate_loss(X[:V], Y[:V]).mean()
            ref.close()
        _oracle_curves.update(out)
    return _oracle_curves


def separation(curves):
    """In units of (beta): per iteration the least distance between two members, and per pair of consecutive iterations the least
    change of a member."""
    it, K = curves.shape
    members = np.array([min(abs(curves[i, a] - curves[i, b]) / max(budget(curves[i, a]), budget(curves[i, b]))
                            for a in range(K) for b in range(a + 1, K)) for i in range(it)])
    steps = np.array([min(abs(curves[i + 1, k] - curves[i, k]) / max(budget(curves[i + 1, k]), budget(curves[i, k]))
                          for k in range(K)) for i in range(it - 1)])
    return members, steps
