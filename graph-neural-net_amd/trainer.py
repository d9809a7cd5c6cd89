"""Host-side mirror of NeuralNetTrainer.java and of MNISTTrainer's data handling, over the C ABI.

NeuralNetTrainer (NNT:11-170): epoch sampler without replacement, `train` loop, 1 % validation
loss with the observer line format "%d,%.2f".  The training set lives in HBM (uploaded once by
the constructor); a sample() draw is a list of row indices, gathered on the GPU.

MNIST side (MNISTTrainer.java): IDX parsing (MT:26-66, 76-118) -- raw bytes go to the GPU, which
applies the reference's encoding (pixel/255.0, one-hot) -- and the accuracy loops with the `>=`
argmax (MT:159-197).
"""
import ctypes as C
import struct

import numpy as np

from . import _capi


class Sampler:
    """NNT:143-168 over dataset row indices (gnn_sampler_* in include/gnn_mlp.h)."""

    def __init__(self, master_size, seed=1):
        self._lib = _capi.load()
        self._h = C.c_void_p()
        _capi.check(self._lib.gnn_sampler_create(int(master_size), int(seed), C.byref(self._h)))
        self.master_size = int(master_size)

    def sample(self, batch_size):
        out = np.empty(int(batch_size), dtype=np.int32)
        n = C.c_int()
        _capi.check(self._lib.gnn_sampler_sample(self._h, int(batch_size), out.ctypes.data_as(C.POINTER(C.c_int32)),
                                                 C.byref(n)))
        return out[:n.value].copy()

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.gnn_sampler_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NeuralNetTrainer:
    """NeuralNetTrainer(Map<double[],double[]> data, NeuralNet net) (NNT:28-43): `data` is given as
    two row-aligned matrices (or raw uint8 pixels + labels); master order = row order."""

    def __init__(self, data_x, data_y, net, raw_u8=False, seed=1, held_out=None):
        """held_out: (x, y), the test rows of MT:98 in the form of the training rows -- uploaded as the net's held-out set."""
        self.net = net
        if raw_u8:
            net.upload_dataset_u8(data_x, data_y)
        else:
            net.upload_dataset(data_x, data_y)
        if held_out is not None:
            (net.upload_held_out_u8 if raw_u8 else net.upload_held_out)(held_out[0], held_out[1])
        self.size = net.dataset_size
        self.sampler = Sampler(self.size, seed)       # random = new Random(1) (NNT:42)

    def train(self, iterations, stepSize, batchSize, momentum, noise=False, monitor=None, observer=None):
        """NNT:60-92.  observer: a text stream receiving "%d,%.2f\\n" % (i, validation loss) per
        iteration (NNT:71); monitor: an object with step() / finish() (ProgressBar)."""
        if not (iterations > 0 and stepSize > 0):
            raise ValueError("iterations and stepSize must be positive (NNT:62)")
        if not (0 < batchSize < self.size):
            raise ValueError("batchSize must be positive and below the data size (NNT:63)")
        validation_size = self.size // 100 + 1                       # NNT:65
        if observer is None and monitor is None:                     # fastest variant, NNT:88-90
            _capi.check(self.net._lib.gnn_mlp_train_sampled(self.net._h, self.sampler._h, int(iterations),
                                                            int(batchSize), float(stepSize), float(momentum),
                                                            int(bool(noise))))
            return
        if observer is None:                                         # only progress monitored, NNT:75-79 has no validation
            done = 0
            while done < iterations:                                 # (the monitor steps in bursts: a device loop per burst)
                n = min(self.OBSERVER_BURST, iterations - done)
                _capi.check(self.net._lib.gnn_mlp_train_sampled(self.net._h, self.sampler._h, n, int(batchSize), float(stepSize),
                                                                float(momentum), int(bool(noise))))
                for _ in range(n):
                    monitor.step()
                done += n
            monitor.finish()
            return
        # observed (NNT:68-72 with a monitor, NNT:75-79 without): gradientStep + validate(validationSize) per iteration, both on
        # the device; the validation losses of a burst come back in ONE readback and are printed in the reference's format
        done = 0
        while done < iterations:
            n = min(self.OBSERVER_BURST, iterations - done) if monitor is not None else iterations - done
            val = np.empty(n)
            _capi.check(self.net._lib.gnn_mlp_train_sampled_observed(
                self.net._h, self.sampler._h, n, int(batchSize), float(stepSize), float(momentum), int(bool(noise)),
                int(validation_size), val.ctypes.data_as(C.POINTER(C.c_double))))
            for k in range(n):
                observer.write("%d,%.2f\n" % (done + k, val[k]))      # NNT:71
                if monitor is not None:
                    monitor.step()
            done += n
        if monitor is not None:
            monitor.finish()

    OBSERVER_BURST = 256   # iterations per device loop when a progress monitor wants to be stepped

    def log_run(self, path, net_dim, iterations, step, batch, momentum):
        """MT:241: appends the run's row to `path` -- testOnTrainingData (MT:180-197) over the training set and testOnTestData
        (MT:159-172) over the held-out set, both on the device, through train_log_row.  Returns (trainAcc, testAcc)."""
        train_acc, test_acc = accuracy(self.net), accuracy(self.net, held_out=True)
        log_test(path, net_dim, iterations, step, batch, momentum, False, train_acc, test_acc)
        return train_acc, test_acc

    def train_stepwise(self, iterations, stepSize, batchSize, momentum, noise=False, observer=None):
        """The observed loop NNT:75-79 one ABI call per action (sample on the host, an indexed step, a validation readback per
        iteration) -- the form `train` had until round 4; kept for the tests that compare the device loop against it."""
        validation_size = self.size // 100 + 1
        for i in range(iterations):
            self.net.gradient_step_indexed(self.sampler.sample(batchSize), stepSize, momentum, noise)
            if observer is not None:
                observer.write("%d,%.2f\n" % (i, self.validate(validation_size)))

    def validate(self, batchSize):
        """NNT:102-113: mean loss over the first batchSize samples in master order.  One call and one readback
        (NeuralNet.evaluate_range): the rows' f32 losses are summed in fp64 on the device, so the value is that of a host sum of
        loss_range over blocks of max_batch up to the fp64 order of the per-row sum."""
        return self.net.evaluate_range(0, batchSize)[1] / batchSize


class NetGroupTrainer:
    """NeuralNetTrainer for a NetGroup: ONE data set and ONE sampler (Random(seed), NNT:42) for every member -- the reference's
    sweep of MNISTTrainer runs, each of which samples with Random(1), as one trainer.  seed: a sequence of K seeds gives
    member k its own sampler Random(seed[k]) -- K independent runs, the sampler's share of a seed-variance study included."""

    OBSERVER_BURST = NeuralNetTrainer.OBSERVER_BURST

    def __init__(self, data_x, data_y, group, raw_u8=False, seed=1, held_out=None):
        """held_out: (x, y), uploaded as the group's held-out set (NeuralNetTrainer)."""
        self.group = group
        if raw_u8:
            group.upload_dataset_u8(data_x, data_y)
        else:
            group.upload_dataset(data_x, data_y)
        if held_out is not None:
            (group.upload_held_out_u8 if raw_u8 else group.upload_held_out)(held_out[0], held_out[1])
        self.size = group._dataset_rows
        if np.ndim(seed) == 0:
            self.sampler = Sampler(self.size, seed)
        else:
            if len(seed) != len(group):
                raise ValueError("seed: one per member (%d), got %d" % (len(group), len(seed)))
            self.sampler = [Sampler(self.size, s) for s in seed]

    def train(self, iterations, stepSizes, batchSize, momenta, noise=False, monitor=None, observers=None):
        """NNT:60-92 for every member (stepSizes / momenta: one value per member, or a scalar for all).  observers: K text
        streams, observers[k] receiving "%d,%.2f\n" % (i, validation loss of member k) per iteration (NNT:71); monitor: an
        object with step() / finish(), stepped once per iteration.  batchSize: an int, or -- a trainer with a seed per member -- a
        sequence of K ints, member k training with batches of batchSize[k] (NetGroup.train_sampled)."""
        if not iterations > 0:
            raise ValueError("iterations must be positive (NNT:62)")
        if np.ndim(batchSize) != 0:
            batchSize = [int(b) for b in batchSize]
            if len(batchSize) != len(self.group):
                raise ValueError("batchSize: one per member (%d), got %d" % (len(self.group), len(batchSize)))
        if not all(0 < b < self.size for b in (batchSize if np.ndim(batchSize) != 0 else [batchSize])):
            raise ValueError("batchSize must be positive and below the data size (NNT:63)")
        if observers is not None and len(observers) != len(self.group):
            raise ValueError("observers: one stream per member (%d), got %d" % (len(self.group), len(observers)))
        validation_size = self.size // 100 + 1                       # NNT:65
        done = 0
        while done < iterations:                                     # (a monitor steps in bursts: a device loop per burst)
            n = min(self.OBSERVER_BURST, iterations - done) if monitor is not None else iterations - done
            if observers is None:
                self.group.train_sampled(self.sampler, n, batchSize, stepSizes, momenta, noise)
            else:
                val = self.group.train_sampled_observed(self.sampler, n, batchSize, stepSizes, momenta, validation_size, noise)
            for i in range(n):
                if observers is not None:
                    for k, o in enumerate(observers):
                        o.write("%d,%.2f\n" % (done + i, val[i, k]))  # NNT:71
                if monitor is not None:
                    monitor.step()
            done += n
        if monitor is not None:
            monitor.finish()


# ---- MNIST (MNISTTrainer.java) ---------------------------------------------------------------
def read_idx_images(path):
    """MT:37-47: magic 2051, count, rows, cols (big-endian int32, MT:76-80), then raw bytes."""
    with open(path, "rb") as f:
        magic, n, rows, cols = struct.unpack(">iiii", f.read(16))
        if magic != 2051:
            raise ValueError("%s: bad IDX image magic %d (MT:39 asserts 2051)" % (path, magic))
        data = np.frombuffer(f.read(n * rows * cols), dtype=np.uint8)
    if data.size != n * rows * cols:
        raise ValueError("%s: truncated" % path)
    return data.reshape(n, rows * cols)


def read_idx_labels(path):
    """MT:38, 40: magic 2049, count, then one byte per label (MT:112-118)."""
    with open(path, "rb") as f:
        magic, n = struct.unpack(">ii", f.read(8))
        if magic != 2049:
            raise ValueError("%s: bad IDX label magic %d (MT:38 asserts 2049)" % (path, magic))
        data = np.frombuffer(f.read(n), dtype=np.uint8)
    if data.size != n:
        raise ValueError("%s: truncated" % path)
    return data


def accuracy(net, labels=None, first=0, n=None, held_out=False):
    """testOnTrainingData / testOnTestData (MT:159-197) over dataset rows [first, first+len):
    hit when the `>=` argmax of propagate() equals the label.  With labels = None the expected classes are the dataset's own
    expected rows (MT:186-188) and the whole loop runs on the device (gnn_mlp_count_hits_range: one readback).
    held_out=True: the rows of the net's held-out set against their own expected rows (testOnTestData, MT:159-172)."""
    if held_out:
        if labels is not None:
            raise ValueError("held_out=True counts against the held-out set's own expected rows")
        n = net.held_out_size - first if n is None else n
        return net.count_hits_range(first, n, held_out=True) / n
    if labels is None:
        n = net.dataset_size - first if n is None else n
        return net.count_hits_range(first, n) / n
    labels = np.asarray(labels)
    hits, off = 0, 0
    while off < labels.size:
        n = min(net.max_batch, labels.size - off)
        hits += int((net.argmax_range(first + off, n) == labels[off:off + n]).sum())
        off += n
    return hits / labels.size


def per_class(conf):
    """(recall[d], precision[d]) of a confusion matrix conf[expected, predicted]: recall[c] = conf[c, c] / (rows expecting c),
    precision[c] = conf[c, c] / (rows predicted c); NaN where that row or column is empty."""
    conf = np.asarray(conf, dtype=np.float64)
    if conf.ndim != 2 or conf.shape[0] != conf.shape[1]:
        raise ValueError("expected a square matrix, got shape %r" % (conf.shape,))
    diag, rows, cols = np.diag(conf), conf.sum(axis=1), conf.sum(axis=0)
    recall = np.where(rows > 0, diag / np.where(rows > 0, rows, 1.0), np.nan)
    precision = np.where(cols > 0, diag / np.where(cols > 0, cols, 1.0), np.nan)
    return recall, precision


def fgsm(net, X, Y, eps, clip=(0.0, 1.0)):
    """The fast-gradient-sign perturbation of the rows: clip(X + eps * sign(g)), g = net.input_gradient(X, Y).  Computed on the
    host, in fp64, for any inner activation (the device holds f(x), not x); clip=None leaves the rows unclipped.  For rows that
    are RESIDENT, non-negative and behind an inner activation that is the identity there (leaky ReLU, ReLU, identity) the device
    forms the same perturbation in f32 without a round trip: NeuralNet.fgsm_range, evaluate_fgsm_range, train_sampled_fgsm."""
    X = np.asarray(X, dtype=np.float64)
    out = X + float(eps) * np.sign(net.input_gradient(X, Y))
    return out if clip is None else np.clip(out, clip[0], clip[1])


def _pgd_mix(u):
    u = u ^ (u >> np.uint32(16))
    u = u * np.uint32(0x7feb352d)
    u = u ^ (u >> np.uint32(15))
    u = u * np.uint32(0x846ca68b)
    return u ^ (u >> np.uint32(16))


def pgd_start(X, eps, clip=(0.0, 1.0), start_seed=0, first_row=0, iteration=0):
    """The random start of the projected attack (include/gnn_mlp.h) in numpy: float32 rows a_0 = clip(x0 + eps * u), u in [-1, 1)
    from the hash of (start_seed, iteration, row index in the resident set, column), uint32 arithmetic that wraps.  first_row: the
    set index of the first row, or one index per row (a sampled batch)."""
    x0 = np.atleast_2d(np.asarray(X, dtype=np.float32))
    rows = np.asarray(first_row, dtype=np.int64)
    rows = (rows + np.arange(x0.shape[0])) if rows.ndim == 0 else rows.reshape(-1)
    if rows.shape[0] != x0.shape[0]:
        raise ValueError("one row index per row")
    with np.errstate(over="ignore"):
        seed = _pgd_mix(np.array([int(start_seed)], dtype=np.uint32)) + np.uint32(int(iteration) & 0xFFFFFFFF)
        r = _pgd_mix(_pgd_mix(seed) ^ (rows & 0xFFFFFFFF).astype(np.uint32))
        h = _pgd_mix(r[:, None] + np.uint32(0x9E3779B9) * np.arange(x0.shape[1], dtype=np.uint32)[None, :])
    u = (h >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -23) - np.float32(1.0)
    v = x0 + np.float32(eps) * u
    return np.minimum(np.maximum(v, np.float32(clip[0])), np.float32(clip[1]))


def pgd(net, X, Y, eps, alpha, steps, clip=(0.0, 1.0), start_seed=None, first_row=0, iteration=0):
    """The projected attack on host rows: `steps` times a + alpha * sign(g), g = net.input_gradient(a, Y), projected onto the
    eps-ball around X and then clipped, from X or (start_seed) from pgd_start's rows; steps=0 returns the start rows clipped.  The
    host route: one synchronising gradient call per step, the formula and the start carried in numpy float32 exactly as the device
    calls define them (NeuralNet.pgd_range, evaluate_pgd_range, train_sampled_pgd), for any inner activation.  first_row and
    iteration key the start as those calls do: the set index of the first row (or one index per row) and the iteration's number."""
    single = np.ndim(X) == 1
    x0 = np.atleast_2d(np.asarray(X, dtype=np.float32))
    Y = np.atleast_2d(np.asarray(Y, dtype=np.float64))
    eps_f, alpha_f, lo, hi = np.float32(eps), np.float32(alpha), np.float32(clip[0]), np.float32(clip[1])
    below, above = x0 - eps_f, x0 + eps_f
    box = lambda a: np.minimum(np.maximum(a, lo), hi)
    if start_seed is not None:
        a = pgd_start(x0, eps, clip, start_seed, first_row, iteration)
    else:
        a = x0 if steps > 0 else box(x0)
    for _ in range(int(steps)):
        g = np.atleast_2d(net.input_gradient(a.astype(np.float64), Y))
        s = (g > 0).astype(np.float32) - (g < 0).astype(np.float32)
        v = a + alpha_f * s
        a = box(np.minimum(np.maximum(v, below), above))
    out = a.astype(np.float64)
    return out[0] if single else out


def integrated_gradients(net, X, Y, steps, baseline=0.0):
    """Integrated gradients of calculateLoss on host rows: (X - baseline) times the mean of net.input_gradient over `steps` midpoints
    a_k = baseline + alpha_k * (X - baseline), alpha_k = float32((k + 0.5) / steps), of the straight path from the baseline (one
    scalar) to the row.  The host route: one synchronising gradient call per point, the formula carried in numpy float32 exactly
    as the device call defines it (NeuralNet.integrated_gradients_range), for any inner activation."""
    single = np.ndim(X) == 1
    x0 = np.atleast_2d(np.asarray(X, dtype=np.float32))
    Y = np.atleast_2d(np.asarray(Y, dtype=np.float64))
    m = int(steps)
    if m < 1:
        raise ValueError("steps must be at least 1")
    b, mf = np.float32(baseline), np.float32(m)
    d = x0 - b
    s = None
    for k in range(m):
        a = b + np.float32((k + 0.5) / m) * d
        g = np.atleast_2d(net.input_gradient(a.astype(np.float64), Y)).astype(np.float32)
        s = g if s is None else s + g
    out = (d * (s / mf)).astype(np.float64)
    return out[0] if single else out


def convergence_delta(net, X, Y, ig, baseline=0.0):
    """The completeness gap of attributions `ig` of rows X, one value per row: sum_i ig[r][i] - (calculateLoss(x_r) -
    calculateLoss(baseline row)), in fp64 from net.calculateLoss in blocks of net.max_batch rows.  Zero up to the path rule's
    error for integrated gradients; what NeuralNet.integrated_gradients_range(delta=True) computes on the device."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    Y = np.atleast_2d(np.asarray(Y, dtype=np.float64))
    ig = np.atleast_2d(np.asarray(ig, dtype=np.float64))
    base = np.full(X.shape, float(np.float32(baseline)))
    mb = int(getattr(net, "max_batch", len(X)))
    lx = np.concatenate([np.atleast_1d(net.calculateLoss(X[o:o + mb], Y[o:o + mb])) for o in range(0, len(X), mb)])
    lb = np.concatenate([np.atleast_1d(net.calculateLoss(base[o:o + mb], Y[o:o + mb])) for o in range(0, len(X), mb)])
    return ig.sum(axis=1) - (lx - lb)


def train_log_row(net_dim, iterations, step_size, batch_size, momentum, noise, training_acc, test_acc):
    """The row MNISTTrainer.logTest appends to logs/trainLog.csv (MT:211-219):
    `dims,iterations,step,batch,momentum,noise,trainAcc,testAcc` in the reference's number formats
    (`%d`, `%.5f`, `%d`, `%.3f`, Java's boolean text, `%.5f,%.5f`)."""
    dims = "-".join(str(int(d)) for d in net_dim)
    return "%s,%d,%.5f,%d,%.3f,%s,%.5f,%.5f\n" % (dims, iterations, step_size, batch_size, momentum,
                                                 "true" if noise else "false", training_acc, test_acc)


def log_test(path, net_dim, iterations, step_size, batch_size, momentum, noise, training_acc, test_acc):
    """Appends one train_log_row to `path` (the reference opens logs/trainLog.csv in append mode, MT:61)."""
    import os
    d = os.path.dirname(str(path))
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, "a") as f:
        f.write(train_log_row(net_dim, iterations, step_size, batch_size, momentum, noise, training_acc, test_acc))
