"""Host-side mirror of the reference's `NeuralNet` operator interface (NeuralNet.java:7-67) and
its two implementations, over the C ABI of include/gnn_mlp.h.

The reference is Java and the image has no JDK, so the literal Java classes with `native`
methods live only as source in INTEGRATION.md / java/; this module is the same interface (same
method names, argument meaning and error behaviour) in Python for the parity tests and the
bench.  Method names follow the Java ones; snake_case aliases are provided.

Every method calls the HIP library; nothing here computes on the CPU.
"""
import ctypes as C

import numpy as np

from . import _capi

ACT_LEAKY_RELU, ACT_SIGMOID, ACT_TANH, ACT_RELU, ACT_IDENTITY = range(5)
OUT_SOFTMAX_CE, OUT_ACT_LOSS = 0, 1
LOSS_HALF_SQUARED = 0
DTYPE_F32, DTYPE_BF16 = 0, 1

_ACT_NAMES = {"leaky_relu": ACT_LEAKY_RELU, "sigmoid": ACT_SIGMOID, "tanh": ACT_TANH,
              "relu": ACT_RELU, "identity": ACT_IDENTITY}


def _act(a):
    if isinstance(a, str):
        return _ACT_NAMES[a]
    return int(a)


def _f64(a, cols):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.ndim == 1:
        a = a.reshape(1, -1)
    if a.ndim != 2 or a.shape[1] != cols:
        # the reference asserts input.length == layerDims[0] (SCE:166)
        raise ValueError("expected rows of length %d, got shape %r" % (cols, a.shape))
    return a


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


SET_TRAIN, SET_HELD_OUT = 0, 1
BEST_LOSS, BEST_HITS = 0, 1
_RULES = {"loss": BEST_LOSS, "hits": BEST_HITS}


def _rule(rule):
    if isinstance(rule, str):
        if rule not in _RULES:
            raise ValueError("rule: 'loss' or 'hits', got %r" % (rule,))
        return _RULES[rule]
    return int(rule)


def best_point(hits, loss, rule="loss"):
    """The point of a held-out curve that train_sampled_held_out keeps (csrc/keep_best_kernel.h), on the host: the running best
    starts as "none" and is decided in point order.  Point p becomes the best under "loss" when its loss is not NaN and (there
    is no best yet, or its loss is strictly lower); under "hits" when there is no best yet, or it has strictly more hits, or
    equal hits and a strictly lower loss (a NaN loss is never lower).  Ties keep the earlier point.  Returns the final best,
    -1 when "loss" never saw a number."""
    hits = np.asarray(hits).ravel()
    loss = np.asarray(loss, dtype=np.float64).ravel()
    if hits.size != loss.size:
        raise ValueError("hits / loss: one value per point each")
    rule = _rule(rule)
    if rule not in (BEST_LOSS, BEST_HITS):
        raise ValueError("rule: 'loss' or 'hits'")
    at = -1
    for p in range(loss.size):
        h, l = int(hits[p]), float(loss[p])
        if rule == BEST_LOSS:
            better = not np.isnan(l) and (at < 0 or l < float(loss[at]))
        else:
            better = at < 0 or h > int(hits[at]) or (h == int(hits[at]) and l < float(loss[at]))
        if better:
            at = p
    return at


def smooth_labels(labels, d_out, eps):
    """Label smoothing on the host: rows (1 - eps) * onehot(label) + eps / d_out, (n, d_out) fp64 -- targets for set_targets."""
    labels = np.asarray(labels).astype(np.int64).ravel()
    d_out, eps = int(d_out), float(eps)
    if labels.size and (labels.min() < 0 or labels.max() >= d_out):
        raise ValueError("labels outside [0, %d)" % d_out)
    if not 0.0 <= eps <= 1.0:
        raise ValueError("eps must lie in [0, 1]")
    out = np.full((labels.size, d_out), eps / d_out, dtype=np.float64)
    out[np.arange(labels.size), labels] += 1.0 - eps
    return out


class NeuralNet:
    """NeuralNet.java:7-67 -- propagate / calculateLoss / calculateWeightGradient /
    gradientStep / getInputDim / getOutputDim, batched: a 2-D array is a batch of rows."""

    def __init__(self, layer_dims, out_kind, inner_act, last_act, loss, seed=1, dtype=DTYPE_F32,
                 device=0, max_batch=1024):
        self._lib = _capi.load()
        self._h = C.c_void_p()
        dims = [int(d) for d in layer_dims]
        arr = (C.c_int32 * len(dims))(*dims)
        _capi.check(self._lib.gnn_mlp_create(arr, len(dims), out_kind, _act(inner_act), _act(last_act),
                                             loss, seed, dtype, device, max_batch, C.byref(self._h)))
        self.layer_dims = dims
        self.max_batch = max_batch
        self.n_params = self._lib.gnn_mlp_num_params(self._h)

    # -- lifetime ---------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.gnn_mlp_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- NeuralNet.java ---------------------------------------------------------------------
    def getInputDim(self):
        return self._lib.gnn_mlp_input_dim(self._h)

    def getOutputDim(self):
        return self._lib.gnn_mlp_output_dim(self._h)

    def propagate(self, input):
        """NN:16.  1-D input -> 1-D output; 2-D -> one output row per input row."""
        single = np.ndim(input) == 1
        X = _f64(input, self.layer_dims[0])
        out = np.empty((X.shape[0], self.layer_dims[-1]))
        _capi.check(self._lib.gnn_mlp_propagate(self._h, _dp(X), X.shape[0], _dp(out)))
        return out[0] if single else out

    def calculateLoss(self, input, expected):
        """NN:27."""
        single = np.ndim(input) == 1
        X = _f64(input, self.layer_dims[0])
        Y = _f64(expected, self.layer_dims[-1])
        if X.shape[0] != Y.shape[0]:
            raise ValueError("input / expected row counts differ")
        out = np.empty(X.shape[0])
        _capi.check(self._lib.gnn_mlp_loss(self._h, _dp(X), _dp(Y), X.shape[0], _dp(out)))
        return float(out[0]) if single else out

    def calculateWeightGradient(self, input, expected):
        """NN:39.  Returns {layer index: ndarray[d_l, d_{l+1}]} like the reference's
        Map<Integer,double[][]>; for a batch the per-sample gradients are summed."""
        X = _f64(input, self.layer_dims[0])
        Y = _f64(expected, self.layer_dims[-1])
        flat = np.empty(self.n_params)
        _capi.check(self._lib.gnn_mlp_weight_gradient(self._h, _dp(X), _dp(Y), X.shape[0], _dp(flat)))
        return self._split(flat)

    def gradientStep(self, batch, step, momentum, noise=False, expected=None):
        """NN:51.  `batch` is either a mapping/sequence of (input, expected) pairs like the
        reference's Map<double[],double[]> (iteration order = row order), or an input matrix
        with `expected` given separately."""
        if expected is None:
            items = list(batch.items()) if hasattr(batch, "items") else list(batch)
            if not items:
                raise ValueError("batch must be non-empty (SCE:300)")
            X = np.stack([np.asarray(k, dtype=np.float64) for k, _ in items])
            Y = np.stack([np.asarray(v, dtype=np.float64) for _, v in items])
        else:
            X, Y = batch, expected
        X = _f64(X, self.layer_dims[0])
        Y = _f64(Y, self.layer_dims[-1])
        if X.shape[0] != Y.shape[0]:
            raise ValueError("input / expected row counts differ")
        _capi.check(self._lib.gnn_mlp_gradient_step(self._h, _dp(X), _dp(Y), X.shape[0], float(step),
                                                    float(momentum), int(bool(noise))))

    # snake_case aliases
    get_input_dim = getInputDim
    get_output_dim = getOutputDim
    calculate_loss = calculateLoss
    calculate_weight_gradient = calculateWeightGradient
    gradient_step = gradientStep

    # -- extensions needed for parity tests (weights are private in the reference, SCE:15) ----
    def argmax(self, input):
        X = _f64(input, self.layer_dims[0])
        out = np.empty(X.shape[0], dtype=np.int32)
        _capi.check(self._lib.gnn_mlp_argmax(self._h, _dp(X), X.shape[0], out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    def _split(self, flat):
        out, off = {}, 0
        for l in range(len(self.layer_dims) - 1):
            n = self.layer_dims[l] * self.layer_dims[l + 1]
            out[l] = flat[off:off + n].reshape(self.layer_dims[l], self.layer_dims[l + 1])
            off += n
        return out

    def get_weights(self):
        flat = np.empty(self.n_params)
        _capi.check(self._lib.gnn_mlp_get_weights(self._h, _dp(flat)))
        return flat

    def set_weights(self, flat):
        flat = np.ascontiguousarray(flat, dtype=np.float64).ravel()
        if flat.size != self.n_params:
            raise ValueError("expected %d weights" % self.n_params)
        _capi.check(self._lib.gnn_mlp_set_weights(self._h, _dp(flat)))

    def get_momentum(self):
        flat = np.empty(self.n_params)
        _capi.check(self._lib.gnn_mlp_get_momentum(self._h, _dp(flat)))
        return flat

    def set_momentum(self, flat):
        flat = np.ascontiguousarray(flat, dtype=np.float64).ravel()
        if flat.size != self.n_params:
            raise ValueError("expected %d values" % self.n_params)
        _capi.check(self._lib.gnn_mlp_set_momentum(self._h, _dp(flat)))

    @property
    def time(self):
        return self._lib.gnn_mlp_time(self._h)

    def save_checkpoint(self, path):
        _capi.check(self._lib.gnn_mlp_save_checkpoint(self._h, str(path).encode()))

    def load_checkpoint(self, path):
        _capi.check(self._lib.gnn_mlp_load_checkpoint(self._h, str(path).encode()))

    # -- device-resident data (the trainer's side of the boundary, NNT:28-43,143-168) ---------
    def upload_dataset(self, X, Y):
        X = _f64(X, self.layer_dims[0])
        Y = _f64(Y, self.layer_dims[-1])
        if X.shape[0] != Y.shape[0]:
            raise ValueError("input / expected row counts differ")
        _capi.check(self._lib.gnn_mlp_upload_dataset(self._h, _dp(X), _dp(Y), X.shape[0]))

    def upload_dataset_u8(self, pixels, labels):
        pixels = np.ascontiguousarray(pixels, dtype=np.uint8).reshape(-1, self.layer_dims[0])
        labels = np.ascontiguousarray(labels, dtype=np.uint8).ravel()
        if pixels.shape[0] != labels.size:
            raise ValueError("pixel / label row counts differ")
        u8 = C.POINTER(C.c_uint8)
        _capi.check(self._lib.gnn_mlp_upload_dataset_u8(self._h, pixels.ctypes.data_as(u8),
                                                        labels.ctypes.data_as(u8), labels.size))

    @property
    def dataset_size(self):
        return self._lib.gnn_mlp_dataset_size(self._h)

    # -- the held-out set (MNISTTrainer's test rows, MT:98, MT:159-172): a second resident set, read by evaluation only -----
    def upload_held_out(self, X, Y):
        X = _f64(X, self.layer_dims[0])
        Y = _f64(Y, self.layer_dims[-1])
        if X.shape[0] != Y.shape[0]:
            raise ValueError("input / expected row counts differ")
        _capi.check(self._lib.gnn_mlp_upload_held_out(self._h, _dp(X), _dp(Y), X.shape[0]))

    def upload_held_out_u8(self, pixels, labels):
        pixels = np.ascontiguousarray(pixels, dtype=np.uint8).reshape(-1, self.layer_dims[0])
        labels = np.ascontiguousarray(labels, dtype=np.uint8).ravel()
        if pixels.shape[0] != labels.size:
            raise ValueError("pixel / label row counts differ")
        u8 = C.POINTER(C.c_uint8)
        _capi.check(self._lib.gnn_mlp_upload_held_out_u8(self._h, pixels.ctypes.data_as(u8),
                                                         labels.ctypes.data_as(u8), labels.size))

    @property
    def held_out_size(self):
        return self._lib.gnn_mlp_set_rows(self._h, SET_HELD_OUT)

    def train_sampled_held_out(self, sampler, iterations, batch, step, momentum, every, held_rows=None, rule="loss", weights=True):
        """train_sampled (NNT:82-90) with the held-out curve (testOnTestData, MT:159-172, along the run) and the best weights
        kept on the device: after every `every` iterations, and after the last one, rows [0, held_rows) of the held-out set
        (default: all) are evaluated.  Returns (hits[P], loss_sums[P], best_point, best_weights) -- best_point by `rule`
        ("loss" or "hits": best_point()), best_weights the flat weights of get_weights() AT that point, or None with
        weights=False or when best_point is -1."""
        if held_rows is None:
            held_rows = self.held_out_size
        p = self._lib.gnn_mlp_held_out_points(int(iterations), int(every))
        hits = np.zeros(max(p, 0), dtype=np.int64)
        loss = np.zeros(max(p, 0), dtype=np.float64)
        best = C.c_int32(-1)
        w = np.empty(self.n_params) if weights else None
        _capi.check(self._lib.gnn_mlp_train_sampled_held_out(
            self._h, sampler._h, int(iterations), int(batch), float(step), float(momentum), 0, int(every), int(held_rows),
            _rule(rule), hits.ctypes.data_as(C.POINTER(C.c_int64)), _dp(loss), C.byref(best), _dp(w) if weights else None))
        return hits, loss, int(best.value), (w if weights and best.value >= 0 else None)

    def train_sampled(self, sampler, iterations, batch, step, momentum, noise=False):
        """The loop NNT:82-90 on the resident rows: `iterations` times { sampler.sample(batch); gradientStep }, on the device."""
        _capi.check(self._lib.gnn_mlp_train_sampled(self._h, sampler._h, int(iterations), int(batch), float(step),
                                                    float(momentum), int(bool(noise))))

    def gradient_step_indexed(self, idx, step, momentum, noise=False):
        idx = np.ascontiguousarray(idx, dtype=np.int32).ravel()
        _capi.check(self._lib.gnn_mlp_gradient_step_indexed(
            self._h, idx.ctypes.data_as(C.POINTER(C.c_int32)), idx.size, float(step), float(momentum),
            int(bool(noise))))

    def gradient_step_range(self, first, B, step, momentum, noise=False):
        _capi.check(self._lib.gnn_mlp_gradient_step_range(self._h, int(first), int(B), float(step),
                                                          float(momentum), int(bool(noise))))

    def train_range(self, first, B, n_steps, step, momentum):
        _capi.check(self._lib.gnn_mlp_train_range(self._h, int(first), int(B), int(n_steps), float(step),
                                                  float(momentum)))

    def loss_range(self, first, B):
        out = np.empty(B)
        _capi.check(self._lib.gnn_mlp_loss_range(self._h, int(first), int(B), _dp(out)))
        return out

    def argmax_range(self, first, B):
        out = np.empty(B, dtype=np.int32)
        _capi.check(self._lib.gnn_mlp_argmax_range(self._h, int(first), int(B),
                                                   out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    def count_hits_range(self, first=0, n=None, held_out=False):
        """testOnTrainingData / testOnTestData (MT:159-197) over dataset rows [first, first + n): the number of rows whose `>=`
        argmax equals the expected class (the last index whose expected value is 1); one readback.  held_out=True: rows of
        the held-out set (MT:159-172)."""
        if held_out:
            return self.evaluate_range(first, n, held_out=True)[0]
        n = self.dataset_size - int(first) if n is None else int(n)
        out = C.c_int64()
        _capi.check(self._lib.gnn_mlp_count_hits_range(self._h, int(first), n, C.byref(out)))
        return out.value

    # the same pass with what it has on the device returned: gnn_mlp_evaluate_range (one call, one readback, any n)
    def _rows(self, first, n, held_out=False):
        first = int(first)
        if n is None:
            size = self.held_out_size if held_out else self.dataset_size
            if size <= 0:
                raise ValueError("n=None needs an uploaded data set")
            n = size - first
        return first, int(n)

    def evaluate_range(self, first=0, n=None, held_out=False):
        """(hits, loss_sum) over dataset rows [first, first + n): count_hits_range's count (MT:159-197) and the sum of
        calculateLoss over the rows (validate(), NNT:102-113, without its division).  held_out=True (here and in
        confusion_range / labels_range): rows of the held-out set (testOnTestData, MT:159-172)."""
        first, n = self._rows(first, n, held_out)
        hits, loss = C.c_int64(), C.c_double()
        _capi.check(self._lib.gnn_mlp_evaluate_set_range(self._h, int(bool(held_out)), first, n, C.byref(hits), C.byref(loss), None, None))
        return hits.value, loss.value

    def confusion_range(self, first=0, n=None, held_out=False):
        """The confusion matrix of the rows, (d_out, d_out) int64: entry [e, p] counts the rows whose expected class (the last
        index whose expected value is 1, MT:186-188) is e and whose `>=` argmax (MT:166-168) is p.  Exact; its trace is
        count_hits_range's count."""
        first, n = self._rows(first, n, held_out)
        d = self.layer_dims[-1]
        conf = np.zeros((d, d), dtype=np.int64)
        _capi.check(self._lib.gnn_mlp_evaluate_set_range(self._h, int(bool(held_out)), first, n, None, None,
                                                         conf.ctypes.data_as(C.POINTER(C.c_int64)), None))
        return conf

    def labels_range(self, first=0, n=None, held_out=False):
        """argmax_range for any number of rows: int32[n], the labels count_hits_range and confusion_range count."""
        first, n = self._rows(first, n, held_out)
        lab = np.empty(max(n, 0), dtype=np.int32)
        _capi.check(self._lib.gnn_mlp_evaluate_set_range(self._h, int(bool(held_out)), first, n, None, None, None,
                                                         lab.ctypes.data_as(C.POINTER(C.c_int32))))
        return lab

    # -- targets of resident rows: csrc/distill.hip ---------------------------------------------------
    def get_targets(self, first=0, n=None, held_out=False):
        """The expected rows [first, first + n) the device holds, (n, d_out): the fp64 of their f32 values."""
        first, n = self._rows(first, n, held_out)
        out = np.empty((max(n, 0), self.layer_dims[-1]), dtype=np.float64)
        _capi.check(self._lib.gnn_mlp_get_targets_range(self._h, int(bool(held_out)), first, n, _dp(out)))
        return out

    def set_targets(self, Y, first=0, held_out=False):
        """Rewrites the expected rows [first, first + len(Y)) in place (label smoothing, a teacher's outputs, free values): the
        handle then behaves bit for bit as if the set had been uploaded with them.  Inputs and look-ahead state are untouched."""
        Y = _f64(Y, self.layer_dims[-1])
        _capi.check(self._lib.gnn_mlp_set_targets_range(self._h, int(bool(held_out)), int(first), Y.shape[0], _dp(Y)))

    def propagate_range(self, first=0, n=None, held_out=False):
        """propagate() (NN:16) over resident rows [first, first + n), (n, d_out): the output rows of evaluate_range's pass, of
        which labels_range is the `>=` argmax; one readback."""
        first, n = self._rows(first, n, held_out)
        out = np.empty((max(n, 0), self.layer_dims[-1]), dtype=np.float64)
        _capi.check(self._lib.gnn_mlp_propagate_set_range(self._h, int(bool(held_out)), first, n, _dp(out)))
        return out

    def distill_from(self, teacher, keep=0.0, first=0, n=None):
        """Blends a teacher's outputs on THIS net's resident input rows into its expected rows, on the device:
        y' = keep * y + (1 - keep) * t in f32 over training rows [first, first + n).  `teacher` is a NeuralNet (t = its
        propagate_range on these rows) or a NetGroup (t = the ensemble's mean output); only input width, output width, inner
        activation, dtype and device must agree.  keep=1 changes nothing, keep=0 stores the teacher's rows.  Accuracy on the
        training set means nothing afterwards (hits follow the last exact 1.0 of a row); the held-out set stays the measure."""
        first, n = self._rows(first, n)
        if isinstance(teacher, NetGroup):
            _capi.check(self._lib.gnn_mlp_group_distill_range(self._h, teacher._h, first, n, float(keep)))
        elif isinstance(teacher, NeuralNet):
            _capi.check(self._lib.gnn_mlp_distill_range(self._h, teacher._h, first, n, float(keep)))
        else:
            raise TypeError("teacher: a NeuralNet or a NetGroup, got %r" % (type(teacher).__name__,))

    # -- which inputs the loss depends on: csrc/input_grad_kernel.h ----------------------------------
    def input_gradient(self, X, Y):
        """d calculateLoss(x, y) / d x (NN:27; SCE:272-278 continued to the input), one row per input row; a 1-D input gets a
        1-D result, as propagate does.  Leaves the gradient buffer holding this batch's weight gradient; changes no weight."""
        single = np.ndim(X) == 1
        X = _f64(X, self.layer_dims[0])
        Y = _f64(Y, self.layer_dims[-1])
        if X.shape[0] != Y.shape[0]:
            raise ValueError("input / expected row counts differ")
        g = np.empty(X.shape)
        _capi.check(self._lib.gnn_mlp_input_gradient(self._h, _dp(X), _dp(Y), X.shape[0], _dp(g)))
        return g[0] if single else g

    def input_gradient_range(self, first=0, n=None, grad=True, saliency=False):
        """The same over dataset rows [first, first + n), any n, in one call: the gradients (n, d_0); with saliency=True
        (saliency (d_out, d_0), class_rows (d_out,)) as well -- saliency[e] is the sum of |gradient| over the rows whose
        expected class (MT:186-188) is e, class_rows[e] their number.  grad=False, saliency=True returns the pair alone."""
        first, n = self._rows(first, n)
        if not grad and not saliency:
            raise ValueError("nothing asked for")
        d0, d = self.layer_dims[0], self.layer_dims[-1]
        g = np.empty((max(n, 0), d0)) if grad else None
        sal = np.zeros((d, d0)) if saliency else None
        rows = np.zeros(d, dtype=np.int64) if saliency else None
        _capi.check(self._lib.gnn_mlp_input_gradient_range(
            self._h, first, n, _dp(g) if grad else None, _dp(sal) if saliency else None,
            rows.ctypes.data_as(C.POINTER(C.c_int64)) if saliency else None))
        if not saliency:
            return g
        return (g, sal, rows) if grad else (sal, rows)

    # -- adversarial rows on the device: csrc/adversarial.hip -----------------------------------------
    # x' = clip(x + eps * sign(input gradient), lo, hi) in f32 on the rows the device holds.  Needs an inner activation that is the
    # identity on non-negative values (leaky ReLU, ReLU, identity), 0 <= lo <= hi, and -- unchecked -- non-negative rows.
    def fgsm_range(self, eps, first=0, n=None, clip=(0.0, 1.0), held_out=False):
        """The perturbed rows [first, first + n), (n, d_0): element for element clip(float32(x) + float32(eps) * sign(g)) with g
        the value input_gradient_range returns; one readback."""
        first, n = self._rows(first, n, held_out)
        out = np.empty((max(n, 0), self.layer_dims[0]), dtype=np.float64)
        _capi.check(self._lib.gnn_mlp_fgsm_set_range(self._h, int(bool(held_out)), first, n, float(eps), float(clip[0]),
                                                     float(clip[1]), _dp(out)))
        return out

    def evaluate_fgsm_range(self, eps, first=0, n=None, clip=(0.0, 1.0), held_out=False):
        """Robust (hits, loss_sum): evaluate_range's counts on the perturbed rows, each block perturbed against the current
        weights and never leaving the device."""
        first, n = self._rows(first, n, held_out)
        hits, loss = C.c_int64(), C.c_double()
        _capi.check(self._lib.gnn_mlp_evaluate_fgsm_set_range(self._h, int(bool(held_out)), first, n, float(eps), float(clip[0]),
                                                              float(clip[1]), C.byref(hits), C.byref(loss)))
        return hits.value, loss.value

    def train_sampled_fgsm(self, sampler, iterations, batch, step, momentum, eps, clip=(0.0, 1.0)):
        """Adversarial training: train_sampled's loop, every iteration stepping on the perturbation of its own batch against the
        weights of that moment."""
        _capi.check(self._lib.gnn_mlp_train_sampled_fgsm(self._h, sampler._h, int(iterations), int(batch), float(step),
                                                         float(momentum), float(eps), float(clip[0]), float(clip[1])))

    # The iterated, projected attack (PGD; BIM with start_seed=None): per step a + alpha * sign(g), projected onto the eps-ball
    # around the resident row, then clipped; start_seed selects a reproducible random start inside the ball (include/gnn_mlp.h).
    @staticmethod
    def _seed(start_seed):
        return -1 if start_seed is None else int(start_seed)

    def pgd_range(self, eps, alpha, steps, first=0, n=None, clip=(0.0, 1.0), held_out=False, start_seed=None):
        """The attacked rows [first, first + n) after `steps` steps, (n, d_0); steps=1, alpha=eps, no start seed is fgsm_range bit
        for bit; steps=0 returns the start rows.  One readback."""
        first, n = self._rows(first, n, held_out)
        out = np.empty((max(n, 0), self.layer_dims[0]), dtype=np.float64)
        _capi.check(self._lib.gnn_mlp_pgd_set_range(self._h, int(bool(held_out)), first, n, float(eps), float(alpha), int(steps),
                                                    self._seed(start_seed), float(clip[0]), float(clip[1]), _dp(out)))
        return out

    def evaluate_pgd_range(self, eps, alpha, steps, first=0, n=None, clip=(0.0, 1.0), held_out=False, start_seed=None, curve=False):
        """Robust (hits, loss_sum) after `steps` steps; curve=True: two arrays of steps + 1 entries, entry t the state after t steps
        (entry 0: the start rows), each what the call with steps=t returns."""
        first, n = self._rows(first, n, held_out)
        steps = int(steps)
        slots = steps + 1 if curve else 1
        hits, loss = np.zeros(max(slots, 1), dtype=np.int64), np.zeros(max(slots, 1), dtype=np.float64)
        _capi.check(self._lib.gnn_mlp_evaluate_pgd_set_range(
            self._h, int(bool(held_out)), first, n, float(eps), float(alpha), steps, self._seed(start_seed), float(clip[0]),
            float(clip[1]), int(bool(curve)), hits.ctypes.data_as(C.POINTER(C.c_int64)), _dp(loss)))
        return (hits, loss) if curve else (int(hits[0]), float(loss[0]))

    def train_sampled_pgd(self, sampler, iterations, batch, step, momentum, eps, alpha, steps, clip=(0.0, 1.0), start_seed=None):
        """Adversarial training with the iterated attack: train_sampled's loop, every iteration stepping on its own batch after
        `steps` projected steps against the weights of that moment."""
        _capi.check(self._lib.gnn_mlp_train_sampled_pgd(self._h, sampler._h, int(iterations), int(batch), float(step),
                                                        float(momentum), float(eps), float(alpha), int(steps),
                                                        self._seed(start_seed), float(clip[0]), float(clip[1])))

    # -- integrated gradients on the device: csrc/input_grad.hip ----------------------------------------
    def integrated_gradients_range(self, steps, baseline=0.0, first=0, n=None, held_out=False, maps=False, delta=False):
        """The attributions (n, d_0) of calculateLoss to the inputs of rows [first, first + n): (x - baseline) times the mean input
        gradient over `steps` midpoints of the straight path from the baseline (one scalar >= 0) to the row, in f32 as
        include/gnn_mlp.h defines it.  maps=True appends (maps (d_out, d_0), class_rows (d_out,)): the sums of |attribution| over
        the rows of each expected class and their numbers; delta=True appends the completeness gap (n,): the row's attributions
        summed minus (calculateLoss(row) - calculateLoss(baseline)).  The domain is fgsm_range's; one readback."""
        first, n = self._rows(first, n, held_out)
        d0, d = self.layer_dims[0], self.layer_dims[-1]
        ig = np.empty((max(n, 0), d0))
        sal = np.zeros((d, d0)) if maps else None
        rows = np.zeros(d, dtype=np.int64) if maps else None
        gap = np.empty(max(n, 0)) if delta else None
        _capi.check(self._lib.gnn_mlp_integrated_gradients_set_range(
            self._h, int(bool(held_out)), first, n, int(steps), float(baseline), _dp(ig), _dp(sal) if maps else None,
            rows.ctypes.data_as(C.POINTER(C.c_int64)) if maps else None, _dp(gap) if delta else None))
        if not maps and not delta:
            return ig
        return (ig,) + ((sal, rows) if maps else ()) + ((gap,) if delta else ())

    # -- data-parallel hooks ------------------------------------------------------------------
    @property
    def grad_elems(self):
        return self._lib.gnn_mlp_grad_elems(self._h)

    def grad_device_ptr(self):
        p = C.c_void_p()
        _capi.check(self._lib.gnn_mlp_grad_device_ptr(self._h, C.byref(p)))
        return p.value

    def bind_grad_buffer(self, dev_ptr, n_elems):
        _capi.check(self._lib.gnn_mlp_bind_grad_buffer(self._h, C.c_void_p(dev_ptr), int(n_elems)))

    def set_stream(self, hip_stream):
        _capi.check(self._lib.gnn_mlp_set_stream(self._h, C.c_void_p(hip_stream or 0)))

    def compute_gradient_range(self, first, B_local):
        _capi.check(self._lib.gnn_mlp_compute_gradient_range(self._h, int(first), int(B_local)))

    def compute_gradient(self, X, Y):
        X = _f64(X, self.layer_dims[0])
        Y = _f64(Y, self.layer_dims[-1])
        _capi.check(self._lib.gnn_mlp_compute_gradient(self._h, _dp(X), _dp(Y), X.shape[0]))

    def apply_update(self, B_global, step, momentum):
        _capi.check(self._lib.gnn_mlp_apply_update(self._h, int(B_global), float(step), float(momentum)))

    # -- one process per GPU, the exchange inside the library's step loop (gnn_mlp_rccl_*) --------
    @staticmethod
    def rccl_unique_id():
        """128 bytes from ncclGetUniqueId: rank 0 makes them, the caller hands them to every rank."""
        buf = C.create_string_buffer(128)
        _capi.check(_capi.load().gnn_mlp_rccl_unique_id(buf))
        return buf.raw

    def rccl_attach(self, unique_id, n_ranks, rank):
        if len(unique_id) != 128:
            raise ValueError("an RCCL unique id is 128 bytes")
        _capi.check(self._lib.gnn_mlp_rccl_attach(self._h, C.c_char_p(bytes(unique_id)), int(n_ranks), int(rank)))

    def rccl_detach(self):
        _capi.check(self._lib.gnn_mlp_rccl_detach(self._h))

    def rccl_train_range(self, first, B_local, n_steps, step, momentum):
        """n_steps global gradientSteps: this rank's rows [first + s B_local, ...) per step, one ncclAllReduce of the flat gradient
        per step inside the call, the identical update with batchSize = B_local * n_ranks."""
        _capi.check(self._lib.gnn_mlp_rccl_train_range(self._h, int(first), int(B_local), int(n_steps), float(step), float(momentum)))

    def hint_next_range(self, first, B):
        """The next gradient computation will run on dataset rows [first, first+B) (speed only)."""
        _capi.check(self._lib.gnn_mlp_hint_next_range(self._h, int(first), int(B)))

    def synchronize(self):
        _capi.check(self._lib.gnn_mlp_synchronize(self._h))

    def forget_lookahead(self):
        """Drop the first-layer sums made ahead for the next batch and any pending hint (results unchanged)."""
        _capi.check(self._lib.gnn_mlp_forget_lookahead(self._h))

    def advance_time(self, steps):
        _capi.check(self._lib.gnn_mlp_advance_time(self._h, int(steps)))

    def recover_stream(self):
        """After a failed stream capture: leave capture mode, drop the sticky HIP error."""
        _capi.check(self._lib.gnn_mlp_recover_stream(self._h))

    # -- shape specialisation -----------------------------------------------------------------
    def specialize(self):
        """Instantiate the fused path's kernels for this net's layer sizes (hiprtc)."""
        _capi.check(self._lib.gnn_mlp_specialize(self._h))
        return self.specialization

    @property
    def specialization(self):
        """0 generic kernels, 1 prebuilt instantiation, 2 instantiated at run time."""
        return self._lib.gnn_mlp_specialization(self._h)

    @property
    def step_launches(self):
        """2 two-launch path, 3 fused three-launch path, 0 per-layer GEMMs."""
        return self._lib.gnn_mlp_step_launches(self._h)

    @property
    def rowblock_state(self):
        """The two-launch step's training kernel: 0 middle4_kernel, 1 rowblock runtime shape, 2 prebuilt, 3 instantiated at run time."""
        return self._lib.gnn_mlp_rowblock_state(self._h)

    @property
    def tile_merge_state(self):
        """The tile kernel's training launch: 0 one tile per workgroup, n > 0 the merged map in a grid of n workgroups."""
        return self._lib.gnn_mlp_tile_merge_state(self._h)

    @property
    def plan_note(self):
        """Why the net is not on the two-launch path ('' when it is)."""
        s = self._lib.gnn_mlp_plan_note(self._h)
        return s.decode() if s else ""

    # -- measurement --------------------------------------------------------------------------
    def timing_enable(self, on=True):
        _capi.check(self._lib.gnn_mlp_timing_enable(self._h, int(bool(on))))

    def timing_read(self, which):
        mean = C.c_double()
        cnt = C.c_int64()
        _capi.check(self._lib.gnn_mlp_timing_read(self._h, int(which), C.byref(mean), C.byref(cnt)))
        return mean.value, cnt.value


class SoftmaxCrossEntropyNeuralNet(NeuralNet):
    """SoftmaxCrossEntropyNeuralNet.java: configurable inner activation, softmax output,
    cross-entropy loss.  ctor SCE:103 takes (layerDims, innerActivationFunc,
    innerActivationPrime); the two lambdas become one `inner_act` enum value (the shipped pair is
    leaky ReLU, MT:234-235)."""

    def __init__(self, layer_dims, inner_act=ACT_LEAKY_RELU, seed=1, dtype=DTYPE_F32, device=0,
                 max_batch=1024):
        super().__init__(layer_dims, OUT_SOFTMAX_CE, inner_act, ACT_IDENTITY, LOSS_HALF_SQUARED,
                         seed=seed, dtype=dtype, device=device, max_batch=max_batch)


class GeneralNeuralNet(NeuralNet):
    """GeneralNeuralNet.java: ctor GNN:112-115 takes (layerDims, inner f, inner f', last f,
    last f', loss, loss'); each (f, f') pair becomes one enum value, (loss, loss') one."""

    def __init__(self, layer_dims, inner_act=ACT_SIGMOID, last_act=ACT_SIGMOID, loss=LOSS_HALF_SQUARED,
                 seed=1, dtype=DTYPE_F32, device=0, max_batch=1024):
        super().__init__(layer_dims, OUT_ACT_LOSS, inner_act, last_act, loss, seed=seed, dtype=dtype,
                         device=device, max_batch=max_batch)


REDUCE_RCCL, REDUCE_DIRECT, REDUCE_DIRECT_RS = 0, 1, 2


class _ReplicaView(NeuralNet):
    """A replica of a DataParallelNeuralNet seen through the single-net interface (borrowed handle:
    closing the view does not destroy it)."""

    def __init__(self, lib, handle, layer_dims, max_batch):
        self._lib, self._h = lib, handle
        self.layer_dims = list(layer_dims)
        self.max_batch = max_batch
        self.n_params = lib.gnn_mlp_num_params(handle)

    def close(self):
        self._h = C.c_void_p()


class _MemberView(_ReplicaView):
    """Member k of a NetGroup through the single-net interface (borrowed handle: closing the view does not destroy it)."""


def _per_member(name, v, k):
    """A scalar for every member, or one value per member."""
    if np.ndim(v) == 0:
        return np.full(k, float(v), dtype=np.float64)
    a = np.ascontiguousarray(v, dtype=np.float64).ravel()
    if a.size != k:
        raise ValueError("%s: one value per member (%d), got %d" % (name, k, a.size))
    return a


class NetGroup:
    """K = len(seeds) nets (1..16) of ONE shape trained side by side over gnn_mlp_group_* (include/gnn_mlp.h): the
    reference's sweeps -- one MNISTTrainer run per step size / momentum / seed -- as one call.  Member k starts from
    Random(seeds[k]) (SCE:139-156) and, after any group call, holds bit for bit what a lone net created with seeds[k]
    holds after the same calls with steps[k], momenta[k].  `members` are borrowed single-net views (propagate,
    count_hits_range, checkpoints, gradientStep ... work on them); the dataset belongs to the group."""

    def __init__(self, layer_dims, seeds, out_kind=OUT_SOFTMAX_CE, inner_act=ACT_LEAKY_RELU, last_act=ACT_IDENTITY,
                 loss=LOSS_HALF_SQUARED, dtype=DTYPE_F32, device=0, max_batch=1024):
        self._lib = _capi.load()
        self._h = C.c_void_p()
        dims = [int(d) for d in layer_dims]
        sd = [int(x) for x in seeds]
        _capi.check(self._lib.gnn_mlp_group_create((C.c_int32 * len(dims))(*dims), len(dims), out_kind, _act(inner_act),
                                                   _act(last_act), loss, (C.c_int64 * max(1, len(sd)))(*sd), len(sd),
                                                   dtype, device, max_batch, C.byref(self._h)))
        self.layer_dims, self.seeds, self.max_batch = dims, sd, max_batch
        self._dataset_rows = None
        self._held_out_rows = None
        self.n_params = sum(dims[l] * dims[l + 1] for l in range(len(dims) - 1))
        self.members = []
        for k in range(len(sd)):
            h = C.c_void_p()
            _capi.check(self._lib.gnn_mlp_group_member(self._h, k, C.byref(h)))
            self.members.append(_MemberView(self._lib, h, dims, max_batch))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            for v in self.members:
                v.close()
            self._lib.gnn_mlp_group_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return len(self.seeds)

    def upload_dataset(self, X, Y):
        X = _f64(X, self.layer_dims[0])
        Y = _f64(Y, self.layer_dims[-1])
        if X.shape[0] != Y.shape[0]:
            raise ValueError("input / expected row counts differ")
        _capi.check(self._lib.gnn_mlp_group_upload_dataset(self._h, _dp(X), _dp(Y), X.shape[0]))
        self._dataset_rows = X.shape[0]

    def upload_dataset_u8(self, pixels, labels):
        pixels = np.ascontiguousarray(pixels, dtype=np.uint8).reshape(-1, self.layer_dims[0])
        labels = np.ascontiguousarray(labels, dtype=np.uint8).ravel()
        if pixels.shape[0] != labels.size:
            raise ValueError("pixel / label row counts differ")
        u8 = C.POINTER(C.c_uint8)
        _capi.check(self._lib.gnn_mlp_group_upload_dataset_u8(self._h, pixels.ctypes.data_as(u8),
                                                              labels.ctypes.data_as(u8), labels.size))
        self._dataset_rows = labels.size

    # the group's held-out set (MT:98, MT:159-172): ONE copy, seen by every member
    def upload_held_out(self, X, Y):
        X = _f64(X, self.layer_dims[0])
        Y = _f64(Y, self.layer_dims[-1])
        if X.shape[0] != Y.shape[0]:
            raise ValueError("input / expected row counts differ")
        _capi.check(self._lib.gnn_mlp_group_upload_held_out(self._h, _dp(X), _dp(Y), X.shape[0]))
        self._held_out_rows = X.shape[0]

    def upload_held_out_u8(self, pixels, labels):
        pixels = np.ascontiguousarray(pixels, dtype=np.uint8).reshape(-1, self.layer_dims[0])
        labels = np.ascontiguousarray(labels, dtype=np.uint8).ravel()
        if pixels.shape[0] != labels.size:
            raise ValueError("pixel / label row counts differ")
        u8 = C.POINTER(C.c_uint8)
        _capi.check(self._lib.gnn_mlp_group_upload_held_out_u8(self._h, pixels.ctypes.data_as(u8),
                                                               labels.ctypes.data_as(u8), labels.size))
        self._held_out_rows = labels.size

    @property
    def held_out_size(self):
        return self.members[0].held_out_size

    def set_targets(self, Y, first=0, held_out=False):
        """NeuralNet.set_targets on the group's ONE copy of the rows (members[k].get_targets reads it)."""
        Y = _f64(Y, self.layer_dims[-1])
        _capi.check(self._lib.gnn_mlp_group_set_targets_range(self._h, int(bool(held_out)), int(first), Y.shape[0], _dp(Y)))

    def train_sampled_held_out(self, samplers, iterations, batches, steps, momenta, every, held_rows=None, rule="loss", weights=True):
        """train_sampled with one sampler and one batch size per member (a scalar `batches`: one size for all), the held-out
        curves (MT:159-172 along the run) and every member's best weights kept on the device (NeuralNet.train_sampled_held_out).
        Returns (hits[P, K], loss_sums[P, K], ensemble_hits[P], best_point[K], best_weights[K, num_params]) -- best_weights None
        with weights=False; row k is unwritten where best_point[k] is -1."""
        k = len(self)
        st, mo = _per_member("steps", steps, k), _per_member("momenta", momenta, k)
        each = self._samplers(samplers)
        if each is None:
            raise ValueError("samplers: one per member")
        bs = [int(batches)] * k if np.ndim(batches) == 0 else [int(b) for b in batches]
        if len(bs) != k:
            raise ValueError("batches: one size per member (%d), got %d" % (k, len(bs)))
        if held_rows is None:
            held_rows = self.held_out_size
        p = max(self._lib.gnn_mlp_held_out_points(int(iterations), int(every)), 0)
        hits = np.zeros((p, k), dtype=np.int64)
        loss = np.zeros((p, k), dtype=np.float64)
        ens = np.zeros(p, dtype=np.int64)
        best = np.full(k, -1, dtype=np.int32)
        w = np.zeros((k, self.n_params)) if weights else None
        i64 = C.POINTER(C.c_int64)
        _capi.check(self._lib.gnn_mlp_group_train_sampled_held_out(
            self._h, each, int(iterations), (C.c_int32 * k)(*bs), _dp(st), _dp(mo), 0, int(every), int(held_rows), _rule(rule),
            hits.ctypes.data_as(i64), _dp(loss), ens.ctypes.data_as(i64), best.ctypes.data_as(C.POINTER(C.c_int32)),
            _dp(w) if weights else None))
        return hits, loss, ens, best, w

    def train_range(self, first, B, n_steps, steps, momenta):
        """NetGroup member k: train_range(first, B, n_steps, steps[k], momenta[k]); scalars apply to every member."""
        st, mo = _per_member("steps", steps, len(self)), _per_member("momenta", momenta, len(self))
        _capi.check(self._lib.gnn_mlp_group_train_range(self._h, int(first), int(B), int(n_steps), _dp(st), _dp(mo)))

    def _samplers(self, sampler):
        """None for ONE sampler (anything with a handle); for a sequence of K samplers, one per member, the handle array."""
        if hasattr(sampler, "_h"):
            return None
        ss = list(sampler)
        if len(ss) != len(self):
            raise ValueError("samplers: one per member (%d), got %d" % (len(self), len(ss)))
        return (C.c_void_p * len(ss))(*[s._h for s in ss])

    def _batches(self, batch, each):
        """None for ONE batch size (an int); for a sequence of K ints, one per member, the int32 array -- which needs one sampler
        per member too: one sampler's draws cannot serve two batch sizes."""
        if np.ndim(batch) == 0:
            return None
        bs = [int(b) for b in batch]
        if len(bs) != len(self):
            raise ValueError("batch: one size per member (%d), got %d" % (len(self), len(bs)))
        if each is None:
            raise ValueError("a batch size per member needs a sampler per member: one sampler's draws cannot serve two batch sizes")
        return (C.c_int32 * len(bs))(*bs)

    def train_sampled(self, sampler, iterations, batch, steps, momenta, noise=False):
        """NNT:82-90 for every member: with the draws of ONE sampler (trainer.Sampler), or, given a sequence of K samplers,
        member k with the draws of sampler[k] -- K independent NeuralNetTrainer runs (gnn_mlp_group_train_sampled_each).
        batch: an int, or with K samplers a sequence of K ints -- member k trains with batches of batch[k]
        (gnn_mlp_group_train_sampled_sizes: the reference's sweep over step AND batch size, logs/trainLog.csv rows 1-3)."""
        st, mo = _per_member("steps", steps, len(self)), _per_member("momenta", momenta, len(self))
        each = self._samplers(sampler)
        sizes = self._batches(batch, each)
        if sizes is not None:
            _capi.check(self._lib.gnn_mlp_group_train_sampled_sizes(self._h, each, int(iterations), sizes, _dp(st), _dp(mo),
                                                                    int(bool(noise)), 0, None))
            return
        if each is not None:
            _capi.check(self._lib.gnn_mlp_group_train_sampled_each(self._h, each, int(iterations), int(batch), _dp(st), _dp(mo),
                                                                   int(bool(noise)), 0, None))
            return
        _capi.check(self._lib.gnn_mlp_group_train_sampled(self._h, sampler._h, int(iterations), int(batch), _dp(st), _dp(mo),
                                                          int(bool(noise))))

    def train_sampled_observed(self, sampler, iterations, batch, steps, momenta, validation_size=None, noise=False):
        """NNT:68-72 / 75-79 for every member with the draws of ONE sampler, or of one sampler per member (a sequence of K):
        train_sampled, and after every iteration validate(validation_size) (NNT:102-113, the mean loss of the first rows of the
        data set; default rows // 100 + 1, NNT:65) of every member.  Returns the curves, an ndarray (iterations, K), from one
        readback.  batch: an int, or with K samplers a sequence of K ints (train_sampled)."""
        st, mo = _per_member("steps", steps, len(self)), _per_member("momenta", momenta, len(self))
        each = self._samplers(sampler)
        sizes = self._batches(batch, each)
        if validation_size is None:
            if getattr(self, "_dataset_rows", None) is None:
                raise ValueError("validation_size=None needs an uploaded data set")
            validation_size = self._dataset_rows // 100 + 1
        val = np.empty((max(int(iterations), 0), len(self)), dtype=np.float64)
        if sizes is not None:
            _capi.check(self._lib.gnn_mlp_group_train_sampled_sizes(self._h, each, int(iterations), sizes, _dp(st), _dp(mo),
                                                                    int(bool(noise)), int(validation_size), _dp(val)))
            return val
        if each is not None:
            _capi.check(self._lib.gnn_mlp_group_train_sampled_each(self._h, each, int(iterations), int(batch), _dp(st), _dp(mo),
                                                                   int(bool(noise)), int(validation_size), _dp(val)))
            return val
        _capi.check(self._lib.gnn_mlp_group_train_sampled_observed(self._h, sampler._h, int(iterations), int(batch), _dp(st), _dp(mo),
                                                                   int(bool(noise)), int(validation_size), _dp(val)))
        return val

    @property
    def sampled_each_iterations(self):
        """(grouped, member_after_member) of the last call with one sampler per member: iterations stepped by the grouped
        launches / member after member (batch sizes that differed at a refill, or a group without grouped launches; with a
        batch size per member every iteration of a group with grouped launches is grouped)."""
        a, b = C.c_int64(), C.c_int64()
        _capi.check(self._lib.gnn_mlp_group_sampled_each_iterations(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    @property
    def observed_launches(self):
        """3: two grouped step launches + one grouped validation launch per iteration; 0: member after member."""
        return self._lib.gnn_mlp_group_observed_launches(self._h)

    @property
    def launches_per_step(self):
        """2: every launch of a group step serves all members; 0: the members are stepped one after another."""
        return self._lib.gnn_mlp_group_launches_per_step(self._h)

    def synchronize(self):
        _capi.check(self._lib.gnn_mlp_group_synchronize(self._h))

    # evaluation of the whole group in one pass (gnn_mlp_group_evaluate_range / _ensemble_range)
    @property
    def eval_launches(self):
        """2: one grouped forward launch + one combine launch per block of rows; 0: member after member."""
        return self._lib.gnn_mlp_group_eval_launches(self._h)

    def _rows(self, first, n, held_out=False):
        first = int(first)
        if n is None:
            rows = getattr(self, "_held_out_rows" if held_out else "_dataset_rows", None)
            if rows is None:
                raise ValueError("n=None needs an uploaded data set")
            n = rows - first
        return first, int(n)

    def evaluate_range(self, first=0, n=None, held_out=False):
        """(hits[K], loss_sums[K], ensemble_hits) over rows [first, first + n) of the group's data set: testOnTrainingData
        (MT:159-197) and the sum of calculateLoss (validate(), NNT:102-113, without its division) for every member, and the
        hits of the ensemble's mean output.  held_out=True (here, in the ensemble calls and in confusion_range): rows of the
        group's held-out set (testOnTestData, MT:159-172)."""
        first, n = self._rows(first, n, held_out)
        k = len(self)
        hits = np.zeros(k, dtype=np.int64)
        loss = np.zeros(k, dtype=np.float64)
        ens = C.c_int64(0)
        _capi.check(self._lib.gnn_mlp_group_evaluate_set_range(self._h, int(bool(held_out)), first, n,
                                                               hits.ctypes.data_as(C.POINTER(C.c_int64)), _dp(loss), C.byref(ens)))
        return hits, loss, int(ens.value)

    def ensemble_propagate_range(self, first, n, held_out=False):
        """The mean of the members' propagate() over the rows: n x d_out (fp64 of the f32 mean, taken in member order)."""
        first, n = self._rows(first, n, held_out)
        out = np.empty((max(n, 0), self.layer_dims[-1]), dtype=np.float64)
        _capi.check(self._lib.gnn_mlp_group_ensemble_set_range(self._h, int(bool(held_out)), first, n, _dp(out), None))
        return out

    def ensemble_argmax_range(self, first, n, held_out=False):
        """argmax (MT:166-168) of the mean output, per row."""
        first, n = self._rows(first, n, held_out)
        lab = np.empty(max(n, 0), dtype=np.int32)
        _capi.check(self._lib.gnn_mlp_group_ensemble_set_range(self._h, int(bool(held_out)), first, n, None,
                                                               lab.ctypes.data_as(C.POINTER(C.c_int32))))
        return lab

    def confusion_range(self, first=0, n=None, labels=False, held_out=False):
        """(member (K, d, d), ensemble (d, d)) int64 confusion matrices over the rows -- entry [e, p]: expected class e (MT:186-188),
        predicted class p, member k's `>=` argmax or the argmax of the mean output -- from the pass of evaluate_range and one
        readback; with labels=True also the members' labels (K, n) int32 the counts were made from."""
        first, n = self._rows(first, n, held_out)
        k, d = len(self), self.layer_dims[-1]
        member = np.zeros((k, d, d), dtype=np.int64)
        ens = np.zeros((d, d), dtype=np.int64)
        lab = np.empty((k, max(n, 0)), dtype=np.int32) if labels else None
        i64 = C.POINTER(C.c_int64)
        _capi.check(self._lib.gnn_mlp_group_confusion_set_range(
            self._h, int(bool(held_out)), first, n, member.ctypes.data_as(i64), ens.ctypes.data_as(i64),
            lab.ctypes.data_as(C.POINTER(C.c_int32)) if labels else None))
        return (member, ens, lab) if labels else (member, ens)

    def input_gradient_range(self, first=0, n=None, members=False, saliency=False):
        """The ensemble's input gradient over the rows, (n, d_0): the mean of the members' gradients (f32, member order, one
        division by K, as ensemble_propagate_range forms the mean output).  members=True: (member (K, n, d_0), ensemble).
        saliency=True appends (ensemble_saliency (d_out, d_0), class_rows (d_out,)), and with members=True the members' maps
        (K, d_out, d_0) in front of them: (member, ensemble, member_saliency, ensemble_saliency, class_rows)."""
        first, n = self._rows(first, n)
        k, d0, d = len(self), self.layer_dims[0], self.layer_dims[-1]
        ens = np.empty((max(n, 0), d0))
        mem = np.empty((k, max(n, 0), d0)) if members else None
        msal = np.zeros((k, d, d0)) if members and saliency else None
        esal = np.zeros((d, d0)) if saliency else None
        rows = np.zeros(d, dtype=np.int64) if saliency else None
        _capi.check(self._lib.gnn_mlp_group_input_gradient_range(
            self._h, first, n, _dp(mem) if mem is not None else None, _dp(ens), _dp(msal) if msal is not None else None,
            _dp(esal) if saliency else None, rows.ctypes.data_as(C.POINTER(C.c_int64)) if saliency else None))
        out = ((mem, ens) if members else (ens,)) + (((msal,) if members else ()) + (esal, rows) if saliency else ())
        return out[0] if len(out) == 1 else out


class DataParallelNeuralNet:
    """The NeuralNet interface over gnn_mlp_dp_* (include/gnn_mlp.h): ONE object, N device replicas,
    gradientStep sharded by rows inside the library (what a single-threaded JVM caller uses; the
    one-process-per-GPU form is data_parallel.py).  propagate / calculateLoss / argmax run on replica 0
    (all replicas are bitwise identical)."""

    def __init__(self, layer_dims, devices=(0,), out_kind=OUT_SOFTMAX_CE, inner_act=ACT_LEAKY_RELU,
                 last_act=ACT_IDENTITY, loss=LOSS_HALF_SQUARED, seed=1, dtype=DTYPE_F32, max_batch=1024,
                 reducer=REDUCE_RCCL):
        self._lib = _capi.load()
        self._h = C.c_void_p()
        dims = [int(d) for d in layer_dims]
        devs = [int(d) for d in devices]
        _capi.check(self._lib.gnn_mlp_dp_create((C.c_int32 * len(dims))(*dims), len(dims), out_kind, _act(inner_act),
                                                _act(last_act), loss, seed, dtype, (C.c_int32 * len(devs))(*devs),
                                                len(devs), max_batch, reducer, C.byref(self._h)))
        self.layer_dims, self.devices, self.max_batch = dims, devs, max_batch
        self.replicas = []
        for r in range(len(devs)):
            h = C.c_void_p()
            _capi.check(self._lib.gnn_mlp_dp_replica(self._h, r, C.byref(h)))
            self.replicas.append(_ReplicaView(self._lib, h, dims, max_batch))
        self.n_params = self.replicas[0].n_params

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            for v in self.replicas:
                v.close()
            self._lib.gnn_mlp_dp_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # NeuralNet.java
    def getInputDim(self):
        return self.layer_dims[0]

    def getOutputDim(self):
        return self.layer_dims[-1]

    def propagate(self, input):
        return self.replicas[0].propagate(input)

    def calculateLoss(self, input, expected):
        return self.replicas[0].calculateLoss(input, expected)

    def calculateWeightGradient(self, input, expected):
        return self.replicas[0].calculateWeightGradient(input, expected)

    def argmax(self, input):
        return self.replicas[0].argmax(input)

    def gradientStep(self, batch, step, momentum, noise=False, expected=None):
        """NN:51, the rows dealt to the replicas in contiguous blocks."""
        if expected is None:
            items = list(batch.items()) if hasattr(batch, "items") else list(batch)
            if not items:
                raise ValueError("batch must be non-empty (SCE:300)")
            X = np.stack([np.asarray(k, dtype=np.float64) for k, _ in items])
            Y = np.stack([np.asarray(v, dtype=np.float64) for _, v in items])
        else:
            X, Y = batch, expected
        X = _f64(X, self.layer_dims[0])
        Y = _f64(Y, self.layer_dims[-1])
        if X.shape[0] != Y.shape[0]:
            raise ValueError("input / expected row counts differ")
        _capi.check(self._lib.gnn_mlp_dp_gradient_step(self._h, _dp(X), _dp(Y), X.shape[0], float(step),
                                                       float(momentum), int(bool(noise))))

    gradient_step = gradientStep

    def upload_dataset(self, X, Y):
        X = _f64(X, self.layer_dims[0])
        Y = _f64(Y, self.layer_dims[-1])
        _capi.check(self._lib.gnn_mlp_dp_upload_dataset(self._h, _dp(X), _dp(Y), X.shape[0]))

    def gradient_step_range(self, first, B, step, momentum, noise=False):
        _capi.check(self._lib.gnn_mlp_dp_gradient_step_range(self._h, int(first), int(B), float(step), float(momentum),
                                                             int(bool(noise))))

    def train_range(self, first, B, n_steps, step, momentum):
        _capi.check(self._lib.gnn_mlp_dp_train_range(self._h, int(first), int(B), int(n_steps), float(step), float(momentum)))

    def set_weights(self, flat):
        flat = np.ascontiguousarray(flat, dtype=np.float64).ravel()
        _capi.check(self._lib.gnn_mlp_dp_set_weights(self._h, _dp(flat)))

    def get_weights(self):
        return self.replicas[0].get_weights()

    def get_momentum(self):
        return self.replicas[0].get_momentum()

    @property
    def time(self):
        return self.replicas[0].time

    def synchronize(self):
        _capi.check(self._lib.gnn_mlp_dp_synchronize(self._h))

    def replicas_identical(self):
        out = C.c_int()
        _capi.check(self._lib.gnn_mlp_dp_replicas_identical(self._h, C.byref(out)))
        return bool(out.value)
