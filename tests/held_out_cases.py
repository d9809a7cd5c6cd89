"""Fixtures of the held-out tests (the held-out set, gnn_mlp_*_set_range, gnn_mlp_train_sampled_held_out and its group form): tiny
nets trained for 123 iterations with a point every 10 -- P = 13, the last point behind 3 iterations -- and what the fp64 oracle says
about their held-out curves.  Computed once per case and shared, never changed.

The cases are drawn so that the best point is decided by more than a GPU run can blur (tests/test_held_out_cpu.py pins that):
T1 / T3 have a loss minimum in the middle of the run with a runner-up more than 1e-3 relative above it; T1h / T2h have so few
held-out rows that several points tie at the maximum of hits and the hits rule is decided by its loss tie-break, with every row's
top-2 margin at every point above 1e-3."""
import numpy as np

LEAKY, SIGMOID, TANH, RELU, IDENTITY = range(5)
SCE, GENERAL = 0, 1
F32, BF16 = 0, 1

TRAIN_ROWS, BATCH, MOMENTUM, ITERATIONS, EVERY = 120, 8, 0.9, 123, 10
POINTS = 13
SEED = 1  # of the net (Random(1), SCE:139-156) and of the sampler (NNT:42)


class Case:
    def __init__(self, name, dims, kind, inner, last, step, held_rows, train_rows=TRAIN_ROWS, dtype=F32):
        self.name, self.dims, self.kind, self.inner, self.last = name, dims, kind, inner, last
        self.step, self.held_rows, self.train_rows, self.dtype = step, held_rows, train_rows, dtype

    def __repr__(self):
        return self.name


_T1 = ([100, 33, 20, 10], SCE, TANH, IDENTITY, 0.02)
CASES = {c.name: c for c in [
    Case("T1", *_T1, 70),
    Case("T1h", *_T1, 6),
    Case("T2h", [60, 40, 12], GENERAL, TANH, SIGMOID, 0.2, 9),
    Case("T3", [24, 136, 10], SCE, LEAKY, IDENTITY, 0.02, 70),
    Case("T1r", *_T1, 70, train_rows=125),        # ragged refill: 125 = 15 * 8 + 5, batches shortened at a refill (NNT:149-155) inside intervals
    Case("T1b", *_T1, 70, dtype=BF16),
]}


def data(dims, n, seed, T):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, dims[0])) * (rng.random((n, dims[0])) < 0.5)
    lab = np.argmax(X @ T + 0.8 * rng.standard_normal((n, dims[-1])), axis=1)
    Y = np.zeros((n, dims[-1]))
    Y[np.arange(n), lab] = 1
    return X, Y


def _teacher(dims):
    return np.random.default_rng(77 + dims[0]).standard_normal((dims[0], dims[-1]))


def training_set(case):
    return data(case.dims, case.train_rows, 5000 + case.dims[0], _teacher(case.dims))


def held_out_set(case, rows=None):
    """The case's held-out rows, drawn at their own count (T1h's six rows are no prefix of T1's seventy)."""
    return data(case.dims, case.held_rows if rows is None else rows, 6000 + case.dims[0], _teacher(case.dims))


def point_iterations(iterations=ITERATIONS, every=EVERY):
    """Iterations (counted from 1) after which a point is taken."""
    P = (iterations + every - 1) // every
    return [min((p + 1) * every, iterations) for p in range(P)]


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


class Curve:
    """The fp64 oracle's run of a case: hits[P], loss[P] (sums) over the held-out rows at every point, margin[P] (the smallest
    top-2 margin of the outputs of any held-out row there) and weights[P] (flat, at every point)."""

    def __init__(self, oracle_mod, case, seed=SEED, step=None, sampler_seed=SEED):
        X, Y = training_set(case)
        Xh, Yh = held_out_set(case)
        X, Xh = f32(X), f32(Xh)  # (the sets are f32 on the device)
        net = oracle_mod.OracleNet(case.dims, out_kind=case.kind, inner_act=case.inner, last_act=case.last, seed=seed)
        net.set_alloc_per_sample(0)
        net.set_weights(f32(net.get_weights()))
        smp = oracle_mod.Sampler(case.train_rows, seed=sampler_seed)
        at = point_iterations()
        expected = np.array([int(np.flatnonzero(r == 1)[-1]) for r in Yh])
        self.hits, self.loss, self.margin, self.weights = [], [], [], []
        for i in range(1, ITERATIONS + 1):
            idx = smp.sample(BATCH)
            net.gradient_step(X[idx], Y[idx], case.step if step is None else step, MOMENTUM)
            if i in at:
                out = net.propagate(Xh)
                lab = np.array([oracle_mod.argmax_rule(r) for r in out])
                srt = np.sort(out, axis=1)
                self.hits.append(int((lab == expected).sum()))
                self.loss.append(float(np.atleast_1d(net.calculate_loss(Xh, Yh)).sum()))
                self.margin.append(float((srt[:, -1] - srt[:, -2]).min()))
                self.weights.append(net.get_weights())
        net.close()
        self.hits, self.loss, self.margin = np.array(self.hits), np.array(self.loss), np.array(self.margin)


_curves = {}


def curve(oracle_mod, name):
    """The oracle's curve of a case: computed once, shared by every test, left unchanged."""
    if name not in _curves:
        _curves[name] = Curve(oracle_mod, CASES[name])
    return _curves[name]
