"""Drawn CALL SEQUENCES (tests/sequence_cases.py) on the device: one handle receives about a hundred calls from the whole ABI
vocabulary, with the dangerous pairs planted (tests/test_sequence_cases_cpu.py pins which), and is compared after EVERY call with
two references that cannot share its mistakes:

the twin (bitwise)   a second handle created under GNN_MLP_DEFER=0 that gets gnn_mlp_forget_lookahead before every call, never a
                     hint, and every loop unrolled into single gradient_step_range / gradient_step_indexed calls on the draws of
                     its own sampler: include/gnn_mlp.h promises that none of this changes a bit.  `time` after every op, every
                     returned array bit for bit, weights and momentum at every checkpoint (sequence_cases.is_checkpoint).  The
                     observed loop's values against the twin's loss_range(0, V).sum() / V within 1e-12 relative (the same f32
                     losses in another fp64 summation order).
the model (fp64)     sequence_cases.Model.  f32: weights and momentum at the checkpoints and at every get_weights / get_momentum
                     within 2e-6 x steps so far, outputs within 2e-4, losses and validation values within 2e-4 relative + 2e-4,
                     labels exact on rows with a top-2 margin above 1e-3 (logits) / 1e-4 (General outputs), hit counts within the
                     count of unsafe rows, confusion matrices exact against numpy counts of the returned labels.
                     bf16: the twin holds the trajectory; every propagate -- one follows a set_weights and a load_checkpoint in
                     every sequence -- within 5e-3 of np_oracle.forward_bf16 on the weights the TWIN reports (reading them does not
                     touch the handle under test), weights and momentum after the first 3 and 5 steps within 2e-4 / 4e-4.
No tolerance here is new (tests/test_parity_gpu.py, tests/test_trainer_gpu.py, tests/test_chain_shapes_gpu.py).  Every assertion
names the sequence, the op index and the op and prints the ops up to it; run_prefix(.., case, n_ops) runs a prefix of a sequence.

The second draw (tests/sequence_cases2.py: input gradients, the held-out set and the keep-best loop, targets and distillation, FGSM)
runs the same way -- run_prefix2, run_group_prefix2 -- with a second handle T, the teacher, and T's own twin.  What is new in the
comparison: perturbed rows are compared in full where the op is clip-only and on adversarial_cases.decided elements where it is signed;
signs and input gradients (held to tests/input_gradient_cases.py's 2e-5 / 4e-3 of the largest element) against the fp64 formulas on
the weights the TWIN reports at that moment; after a distill the targets the device holds are checked against the model's blend
(2e-4 x (1 - keep); bf16: 5e-3 x (1 - keep) on the twin's weights) and then become the model's; the keep-best loop's curves, best
point and best weights are the twin's evaluate_range / get_weights at each point, and the model's within the budgets of losses, hits
and weights.  On the MI355X a case of the second draw takes at most 1.3 s."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import chain_cases as cc
from tests import np_oracle
from tests import adversarial_cases as ac
from tests import sequence_cases as sq
from tests import sequence_cases2 as s2
from tests.test_chain_shapes_gpu import _forced_path as chain_forced_path

pytestmark = pytest.mark.gpu

BAD_ARG = 1
SLAB_NOTE = "more than 16 first-layer K slabs"


def _forced_path():
    return chain_forced_path() or bool(os.environ.get("GNN_MLP_DEFER"))


def _net(gnn, case, seed=1):
    dt = gnn.DTYPE_BF16 if case["dtype"] == "bf16" else gnn.DTYPE_F32
    if case["out_kind"] == cc.OUT_SOFTMAX_CE:
        return gnn.SoftmaxCrossEntropyNeuralNet(case["dims"], inner_act=case["inner"], seed=seed, dtype=dt, max_batch=sq.MAX_BATCH)
    return gnn.GeneralNeuralNet(case["dims"], inner_act=case["inner"], last_act=case["last"], seed=seed, dtype=dt, max_batch=sq.MAX_BATCH)


def _twin(gnn, monkeypatch, case, seed=1):
    with monkeypatch.context() as m:
        m.setenv("GNN_MLP_DEFER", "0")
        return _net(gnn, case, seed)


class _Fail(AssertionError):
    pass


class _Side:
    """one handle with its sampler and its checkpoint files"""

    def __init__(self, gnn, net, tag, tmp, twin, step=cc.STEP, momentum=cc.MOMENTUM):
        self.gnn, self.net, self.tag, self.tmp, self.twin, self.step, self.mom = gnn, net, tag, tmp, twin, step, momentum
        self.sampler = self.each = None
        self.each_seed = 2
        self.N = 0

    def upload(self, X, Y, group=None):
        if group is None:
            self.net.upload_dataset(X, Y)
        if len(X) != self.N:
            for x in (self.sampler, self.each):
                if x is not None: x.close()
            self.sampler = self.gnn.Sampler(len(X), seed=sq.SAMPLER_SEED)
            self.each = self.gnn.Sampler(len(X), seed=self.each_seed)
        self.N, self.X, self.Y = len(X), X, Y

    def close(self):
        for x in (self.sampler, self.each):
            if x is not None: x.close()
        self.net.close()

    def _val(self, V):
        return np.concatenate([self.net.loss_range(o, min(sq.MAX_BATCH, V - o)) for o in range(0, V, sq.MAX_BATCH)]).sum() / V

    def refused(self, kind, variant, Xh, Yh):
        net, N = self.net, self.N
        if kind == "batch":
            call = (lambda: net.gradient_step_range(0, sq.MAX_BATCH + 1, self.step, self.mom)) if variant else \
                   (lambda: net.gradientStep(Xh[:sq.MAX_BATCH + 1], self.step, self.mom, False, expected=Yh[:sq.MAX_BATCH + 1]))
        elif kind == "step":
            call = (lambda: net.gradient_step_range(0, 16, 0.0, self.mom)) if variant else \
                   (lambda: net.gradientStep(Xh[:5], -1.0, self.mom, False, expected=Yh[:5]))
        elif kind == "rows":
            call = (lambda: net.gradient_step_range(N - 10, 16, self.step, self.mom)) if variant else (lambda: net.loss_range(N - 3, 5))
        elif kind == "validation":
            val = np.empty(2)
            call = lambda: self.gnn._capi.check(net._lib.gnn_mlp_train_sampled_observed(
                net._h, self.sampler._h, 2, 16, self.step, self.mom, 0, N + 1, val.ctypes.data_as(C.POINTER(C.c_double))))
        elif kind == "upload":                                       # a group's member trains on the group's data set
            call = lambda: net.upload_dataset(self.X[:20], self.Y[:20])
        try:
            call()
        except self.gnn.GnnError as e:
            return {"code": np.array(e.code)}
        return {"code": np.array(0)}

    def do(self, name, kw, Xh, Yh, i):
        """the op on this handle; what it returned, as {name: array}"""
        net, twin, st, mo = self.net, self.twin, self.step, self.mom
        rows = lambda: (Xh[kw["off"]:kw["off"] + kw["n"]], Yh[kw["off"]:kw["off"] + kw["n"]])
        if twin:
            net.forget_lookahead()
        if name == "step_host":
            X, Y = rows(); net.gradientStep(X, st, mo, False, expected=Y)
        elif name == "step_range":
            net.gradient_step_range(kw["first"], kw["n"], st, mo)
        elif name == "step_indexed":
            net.gradient_step_indexed(np.asarray(kw["idx"], dtype=np.int32), st, mo)
        elif name == "train_range":
            if not twin:
                net.train_range(kw["first"], kw["B"], kw["n_steps"], st, mo)
            else:
                for r in cc.range_batches(self.N, kw["B"], kw["first"], kw["n_steps"]):
                    net.forget_lookahead(); net.gradient_step_range(r, kw["B"], st, mo)
        elif name in ("train_sampled", "train_observed"):
            observed = name == "train_observed"
            if not twin and not observed:
                smp = self.each if kw.get("each") else self.sampler
                self.gnn._capi.check(net._lib.gnn_mlp_train_sampled(net._h, smp._h, kw["iters"], kw["B"], st, mo, 0))
            elif not twin:
                val = np.empty(kw["iters"])
                self.gnn._capi.check(net._lib.gnn_mlp_train_sampled_observed(net._h, self.sampler._h, kw["iters"], kw["B"], st, mo, 0, kw["V"],
                                                                        val.ctypes.data_as(C.POINTER(C.c_double))))
                return {"val": val}
            else:
                val = []
                for _ in range(kw["iters"]):
                    net.forget_lookahead(); net.gradient_step_indexed(self.sampler.sample(kw["B"]), st, mo)
                    if observed:
                        net.forget_lookahead(); val.append(self._val(kw["V"]))
                if observed:
                    return {"val": np.array(val)}
        elif name == "sample":
            return {"idx": self.sampler.sample(kw["B"])}
        elif name == "compute_gradient_range":
            net.compute_gradient_range(kw["first"], kw["n"])
        elif name == "apply_update":
            net.apply_update(kw["B"], st, mo)
        elif name == "hint":
            if not twin: net.hint_next_range(kw["first"], kw["n"])
        elif name == "propagate":
            return {"out": net.propagate(rows()[0])}
        elif name == "loss":
            return {"loss": np.atleast_1d(net.calculateLoss(*rows()))}
        elif name == "argmax":
            return {"labels": net.argmax(rows()[0])}
        elif name == "loss_range":
            return {"loss": net.loss_range(kw["first"], kw["n"])}
        elif name == "argmax_range":
            return {"labels": net.argmax_range(kw["first"], kw["n"])}
        elif name == "count_hits":
            return {"hits": np.array(net.count_hits_range(kw["first"], kw["n"]))}
        elif name == "evaluate":
            hits, loss = net.evaluate_range(kw["first"], kw["n"])
            return {"hits": np.array(hits), "loss_sum": np.array(loss)}
        elif name == "confusion":
            return {"confusion": net.confusion_range(kw["first"], kw["n"]), "labels": net.labels_range(kw["first"], kw["n"])}
        elif name == "labels":
            return {"labels": net.labels_range(kw["first"], kw["n"])}
        elif name == "weight_gradient":
            g = net.calculateWeightGradient(*rows())
            return {"grad": np.concatenate([g[l].ravel() for l in sorted(g)])}
        elif name == "get_weights":
            return {"W": net.get_weights()}
        elif name == "get_momentum":
            return {"V": net.get_momentum()}
        elif name == "save":
            net.save_checkpoint(os.path.join(self.tmp, "%s-%d.ckpt" % (self.tag, kw["slot"])))
        elif name == "load":
            net.load_checkpoint(os.path.join(self.tmp, "%s-%d.ckpt" % (self.tag, kw["slot"])))
        elif name == "set_weights":
            net.set_weights(kw["_W"])
        elif name == "set_momentum":
            net.set_momentum(kw["_V"])
        elif name == "specialize":
            net.specialize()
        elif name == "forget":
            net.forget_lookahead()
        elif name == "advance_time":
            net.advance_time(kw["n"])
        elif name == "timing":
            net.timing_enable(kw["on"])
        elif name == "synchronize":
            net.synchronize()
        elif name == "refused":
            return self.refused(kw["kind"], i % 2, Xh, Yh)
        else:
            raise ValueError(name)
        return {}


def _ctx(case, ops, i):
    return "sequence %s, op %d %r\nops so far:\n%s" % (case["id"], i, ops[i], "\n".join("  %3d %s %r" % (j, o[0], o[1]) for j, o in enumerate(ops[:i + 1])))


def _same(a, b, what, ctx):
    if not np.array_equal(a, b):
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        bad = np.flatnonzero(a.ravel() != b.ravel()) if a.shape == b.shape else []
        raise _Fail("%s differs from the twin's: %d of %d elements, max %.3g\n%s"
                    % (what, len(bad), a.size, np.abs(a - b).max() if a.shape == b.shape else np.nan, ctx))


class _Budget:
    """the largest fraction of each budget a sequence used"""

    def __init__(self):
        self.used = {}

    def check(self, what, err, budget, ctx):
        frac = float(np.max(np.asarray(err, dtype=np.float64) / budget)) if np.size(err) else 0.0
        self.used[what] = max(self.used.get(what, 0.0), frac)
        if not frac <= 1.0:
            raise _Fail("%s: %.3g of the budget\n%s" % (what, frac, ctx))

    def line(self):
        return "  ".join("%s %.3f" % (k, v) for k, v in sorted(self.used.items()))


def _against_model(bud, case, name, got, want, steps, ctx):
    """f32: what op `name` returned against the fp64 model"""
    w_budget = sq.W_ATOL * max(steps, 1)
    if "W" in got and "W" in want: bud.check("weights", np.abs(got["W"] - want["W"]).max(), w_budget, ctx)
    if "V" in got and "V" in want: bud.check("momentum", np.abs(got["V"] - want["V"]).max(), w_budget, ctx)
    if "out" in got: bud.check("outputs", np.abs(got["out"] - want["out"]).max(), sq.OUT_ATOL, ctx)
    if "loss" in got: bud.check("losses", np.abs(got["loss"] - want["loss"]), sq.LOSS_RTOL * np.abs(want["loss"]) + sq.LOSS_ATOL, ctx)
    if "val" in got: bud.check("validation", np.abs(got["val"] - want["val"]), sq.LOSS_RTOL * np.abs(want["val"]) + sq.LOSS_ATOL, ctx)
    if "loss_sum" in got:
        n = want["safe"].size
        bud.check("validation", abs(got["loss_sum"] - want["loss_sum"]) / n, sq.LOSS_RTOL * abs(want["loss_sum"]) / n + sq.LOSS_ATOL, ctx)
    if "labels" in got and "labels" in want:
        safe = want["safe"]
        if not np.array_equal(got["labels"][safe], want["labels"][safe]):
            raise _Fail("labels differ from the oracle's on %d safe rows\n%s" % ((got["labels"][safe] != want["labels"][safe]).sum(), ctx))
    if "hits" in got:
        if abs(int(got["hits"]) - want["hits"]) > want["unsafe"]:
            raise _Fail("hits %d, the oracle's %d, %d unsafe rows\n%s" % (got["hits"], want["hits"], want["unsafe"], ctx))
    if "idx" in got and not np.array_equal(got["idx"], want["idx"]):
        raise _Fail("the sampler's draw differs from the oracle sampler's\n%s" % ctx)


def _confusion_of(labels, Y):
    d = Y.shape[1]
    conf = np.zeros((d, d), dtype=np.int64)
    for lab, y in zip(labels, Y):
        conf[np.flatnonzero(y == 1)[-1], lab] += 1
    return conf


def run_prefix(gnn, oracle_mod, monkeypatch, tmp_path, case, n_ops=None):
    """The first n_ops ops of a lone sequence on a fresh handle and its twin, with every check; returns the budget fractions used.
    A failing assertion names its op index i: run_prefix(.., i + 1) still fails, and shorter prefixes show where it starts."""
    ops = case["ops"][:n_ops]
    bf16 = case["dtype"] == "bf16"
    dims = case["dims"]
    Xh, Yh = sq.host_pool(case["seed"], dims[0], dims[-1])
    w0 = sq.start_weights(oracle_mod, dims)
    Wnew, Vnew = sq.replacement_weights(oracle_mod, dims), sq.replacement_momentum(oracle_mod, dims)
    a = _Side(gnn, _net(gnn, case), "a", str(tmp_path), False)
    b = _Side(gnn, _twin(gnn, monkeypatch, case), "b", str(tmp_path), True)
    model = sq.Model(oracle_mod, case, reads=not bf16)
    bud = _Budget()
    X, Y = sq.dataset(case["seed"], 0, dims[0], dims[-1])
    for s in (a, b):
        s.net.set_weights(w0); s.upload(X, Y)
    assert np.array_equal(a.net.get_weights(), w0)
    first_at = {}
    try:
        for i, (name, kw) in enumerate(ops):
            ctx = _ctx(case, ops, i)
            if name == "upload":
                X, Y = sq.dataset(case["seed"], kw["which"], dims[0], dims[-1])
                b.net.forget_lookahead()
                a.upload(X, Y); b.upload(X, Y)
                got = twin = {}
            else:
                kw = dict(kw, _W=Wnew, _V=Vnew) if name in ("set_weights", "set_momentum") else kw
                got, twin = a.do(name, kw, Xh, Yh, i), b.do(name, kw, Xh, Yh, i)
            want = model.apply(i, (name, kw))
            # the twin: time, and every returned array bit for bit
            if not a.net.time == b.net.time == want["time"]:
                raise _Fail("time %d, the twin's %d, the model's %d\n%s" % (a.net.time, b.net.time, want["time"], ctx))
            for k in got:
                if k == "val":
                    if not np.all(np.abs(got[k] - twin[k]) <= 1e-12 * np.abs(twin[k])):
                        raise _Fail("validation values differ from the twin's by %.3g relative\n%s" % (np.abs(got[k] / twin[k] - 1).max(), ctx))
                else:
                    _same(got[k], twin[k], k, ctx)
            if name == "refused" and int(got["code"]) != BAD_ARG:
                raise _Fail("the refused call returned %d\n%s" % (got["code"], ctx))
            if "confusion" in got:
                f, n = kw["first"], kw["n"]
                if not np.array_equal(got["confusion"], _confusion_of(got["labels"], a.Y[f:f + n])):
                    raise _Fail("the confusion matrix is not the count of the returned labels\n%s" % ctx)
            if sq.is_checkpoint(i, ops):
                got = dict(got, W=a.net.get_weights(), V=a.net.get_momentum())
                _same(got["W"], b.net.get_weights(), "weights", ctx)
                _same(got["V"], b.net.get_momentum(), "momentum", ctx)
                want = dict(want, W=model.W, V=model.V)
            # the model
            if not bf16:
                _against_model(bud, case, name, got, want, want["steps"], ctx)
            else:
                if name == "propagate":
                    ref = np_oracle.forward_bf16(np_oracle.split(b.net.get_weights(), dims), Xh[kw["off"]:kw["off"] + kw["n"]],
                                                 case["inner"], case["out_kind"], case["last"])[2]
                    bud.check("outputs (bf16)", np.abs(got["out"] - ref).max(), sq.BF16_OUT, ctx)
                if "idx" in got and not np.array_equal(got["idx"], want["idx"]):
                    raise _Fail("the sampler's draw differs from the oracle sampler's\n%s" % ctx)
                n = want["steps"]
                if n in sq.BF16_W and n not in first_at:
                    first_at[n] = i
                    bud.check("weights after %d steps (bf16)" % n, np.abs(a.net.get_weights() - model.W).max(), sq.BF16_W[n], ctx)
                    bud.check("momentum after %d steps (bf16)" % n, np.abs(a.net.get_momentum() - model.V).max(), sq.BF16_W[n], ctx)
    finally:
        for s in (a, b):
            s.close()
    return bud.used


@pytest.mark.parametrize("i", range(sq.N_LONE), ids=[sq.lone_case(i)["id"] for i in range(sq.N_LONE)])
def test_lone_sequences(gnn, oracle_mod, monkeypatch, tmp_path, i):
    if _forced_path():
        pytest.skip("path forced by the environment")
    case = sq.lone_case(i)
    used = run_prefix(gnn, oracle_mod, monkeypatch, tmp_path, case)
    print("call-sequence %s (%d ops): largest fraction of each budget used: %s"
          % (case["id"], len(case["ops"]), "  ".join("%s %.3f" % (k, v) for k, v in sorted(used.items()))))


def test_the_sequences_run_on_the_kernels_they_are_for(gnn):
    """The eight nets were chosen by the path they take; read from fresh handles (conditions on the choice, not measurements)."""
    if _forced_path():
        pytest.skip("path forced by the environment")
    path = {}
    for i in range(0, sq.N_LONE, sq.SEEDS_PER_NET):
        case = sq.lone_case(i)
        net = _net(gnn, case)
        if case["net"] == "f32-general": p_dims = case["dims"]
        path[case["net"]] = (len(case["dims"]), net.step_launches, net.rowblock_state, net.specialization, net.plan_note, case["out_kind"])
        net.close()
    p = path
    assert p["f32-rowblock"][1:3] == (2, 1) and p["f32-rowblock"][3] == 0, p          # two launches, row-block kernel, runtime shape
    assert p["f32-middle4"][1:3] == (2, 0), p                                          # two launches, middle4_kernel as the row kernel
    assert p["f32-three-launch"][1] == 3 and SLAB_NOTE in p["f32-three-launch"][4], p
    assert p["f32-per-layer"][1] == 0, p
    assert p["f32-prebuilt"][3] == 1, p
    assert p["f32-general"][1] == 2 and p["f32-general"][5] == cc.OUT_ACT_LOSS, p
    assert p["bf16-rowblock"][0] in (3, 4) and p["bf16-rowblock"][1] == 2 and p["bf16-rowblock"][2] != 0, p
    assert p["bf16-middle4"][0] in (5, 6) and p["bf16-middle4"][1] == 2 and p["bf16-middle4"][2] == 0, p
    for name in p:                                                                     # each class occurs SEEDS_PER_NET times
        assert sum(1 for i in range(sq.N_LONE) if sq.lone_case(i)["net"] == name) == sq.SEEDS_PER_NET
    # the second draw runs on the same eight and on a ninth: the General output head behind a leaky inner activation, two launches
    assert [n[:6] for n in s2.NETS[:len(sq.NETS)]] == [n[:6] for n in sq.NETS]
    case = s2.lone_case(s2.N_LONE - 1)
    net = _net(gnn, case)
    ninth = (net.step_launches, case["out_kind"], case["inner"], case["last"], case["dims"])
    net.close()
    assert ninth == (2, cc.OUT_ACT_LOSS, sq.LEAKY, sq.SIGMOID, p_dims), ninth


# ---- the second draw: the calls merged since the first (tests/sequence_cases2.py) -------------------------------------------------
STATE, UNSUPPORTED = 5, 3
REFUSED2 = {"no_held_out": STATE, "fgsm": UNSUPPORTED, "distill_dims": BAD_ARG, "targets_rows": BAD_ARG}


class _Side2(_Side):
    """a _Side with the second draw's ops.  The twin stays free of look-ahead and of every device-side loop: train_held_out and
    train_fgsm unrolled into single steps with the points and the perturbation made on the host, distill by the host route
    (the teacher's propagate_range on the student's rows as ITS held-out set, the blend in numpy float32, set_targets)."""

    def __init__(self, gnn, net, tag, tmp, twin, case, make):
        super().__init__(gnn, net, tag, tmp, twin)
        self.case, self.make = case, make                      # make(case, seed): a handle of this side's kind
        self.T = self.G = self.odd = None
        self.Xo = self.Yo = None

    def teacher(self, oracle_mod):
        tc = s2.teacher_case(self.case)
        self.T = _Side(self.gnn, self.make(tc, 4), self.tag + "T", self.tmp, self.twin)
        self.T.net.set_weights(sq.start_weights(oracle_mod, tc["dims"], seed=4))
        self.T.upload(*sq.dataset(tc["seed"], 0, tc["dims"][0], tc["dims"][-1]))
        self.T_host = sq.host_pool(tc["seed"], tc["dims"][0], tc["dims"][-1])
        self.group_W = [sq.start_weights(oracle_mod, self.case["dims"], seed=k) for k in s2.GROUP_SEEDS]

    def group(self):
        if self.G is None:
            self.G = _group(self.gnn, dict(self.case, wseeds=list(s2.GROUP_SEEDS)))
            for m, w in zip(self.G.members, self.group_W):
                m.set_weights(w)
        return self.G

    def close(self):
        if self.T is not None: self.T.close()
        if self.G is not None: self.G.close()
        if self.odd is not None: self.odd.close()
        super().close()

    def _code(self, call):
        try:
            call()
        except self.gnn.GnnError as e:
            return {"code": np.array(e.code)}
        return {"code": np.array(0)}

    def refused2(self, kw, Xh, Yh):
        net, kind, d = self.net, kw["kind"], self.case["dims"]
        if kind == "no_held_out":
            return self._code(lambda: net.train_sampled_held_out(self.sampler, 2, 16, self.step, self.mom, 1, 1))
        if kind == "fgsm":
            if kw["call"] == "train_fgsm": return self._code(lambda: net.train_sampled_fgsm(self.sampler, 2, 16, self.step, self.mom, 0.1))
            if kw["call"] == "evaluate_fgsm": return self._code(lambda: net.evaluate_fgsm_range(0.1, 0, 5))
            return self._code(lambda: net.fgsm_range(0.1, 0, 5))
        if kind == "distill_dims":
            if self.odd is None: self.odd = self.make(dict(self.case, dims=[d[0] + 1, 8, d[-1]]), 1)
            return self._code(lambda: net.distill_from(self.odd, 0.5, 0, 5))
        return self._code(lambda: net.set_targets(Yh[:5], first=self.N - 3))

    def _retarget(self, first, n):
        Y = np.array(self.Y)
        Y[first:first + n] = self.net.get_targets(first, n)
        self.Y = Y
        return {"targets": Y[first:first + n].copy()}

    def do(self, name, kw, Xh, Yh, i):
        gnn, net, twin, st, mo = self.gnn, self.net, self.twin, self.step, self.mom
        if name == "teacher":
            return {"T" + k: v for k, v in self.T.do(kw["op"][0], kw["op"][1], self.T_host[0], self.T_host[1], i).items()}
        if name not in s2.NEW_OPS:
            return super().do(name, kw, Xh, Yh, i)
        if twin:
            net.forget_lookahead()
        f, n, held = kw.get("first"), kw.get("n"), bool(kw.get("held"))
        if name == "input_gradient":
            return {"grad_in": net.input_gradient(Xh[kw["off"]:kw["off"] + n], Yh[kw["off"]:kw["off"] + n])}
        if name == "input_gradient_range":
            return {"grad_in": net.input_gradient_range(f, n)}
        if name == "get_targets":
            return {"targets": net.get_targets(f, n, held_out=held)}
        if name == "propagate_set":
            return {"out": net.propagate_range(f, n, held_out=held)}
        if name == "evaluate_set":
            if kw["kind"] == "evaluate":
                hits, loss = net.evaluate_range(f, n, held_out=held)
                return {"hits": np.array(hits), "loss_sum": np.array(loss)}
            lab = {"labels": net.labels_range(f, n, held_out=held)}
            return dict(lab, confusion=net.confusion_range(f, n, held_out=held)) if kw["kind"] == "confusion" else lab
        if name == "fgsm_range":
            p = s2.SIGNED if kw["signed"] else s2.CLIP_ONLY
            return {"rows": net.fgsm_range(p["eps"], f, n, clip=p["clip"], held_out=held)}
        if name == "evaluate_fgsm":
            hits, loss = net.evaluate_fgsm_range(s2.CLIP_ONLY["eps"], f, n, clip=s2.CLIP_ONLY["clip"], held_out=held)
            return {"hits": np.array(hits), "loss_sum": np.array(loss)}
        if name == "upload_held_out":
            self.Xo, self.Yo = s2.held_set(self.case["seed"], kw["size"], self.case["dims"][0], self.case["dims"][-1])
            net.upload_held_out(self.Xo, self.Yo)
        elif name == "set_targets":
            net.set_targets(s2.target_rows(self.case["seed"], kw["tseed"], n, self.case["dims"][-1]), first=f)
            self._retarget(f, n)
        elif name == "distill":
            who, keep = kw["teacher"], kw["keep"]
            if not twin:
                net.distill_from(net if who == "self" else self.T.net if who == "other" else self.group(), keep, f, n)
            else:
                if who == "self":
                    t = net.propagate_range(f, n)
                elif who == "other":
                    self.T.net.forget_lookahead(); self.T.net.upload_held_out(self.X, self.Y)
                    self.T.net.forget_lookahead(); t = self.T.net.propagate_range(f, n, held_out=True)
                else:
                    self.group().upload_held_out(self.X, self.Y)
                    t = self.group().ensemble_propagate_range(f, n, held_out=True)
                k32 = np.float32(keep)
                y = net.get_targets(f, n).astype(np.float32)
                blend = k32 * y + (np.float32(1) - k32) * t.astype(np.float32)      # (numpy rounds each product on its own)
                net.forget_lookahead(); net.set_targets(blend.astype(np.float64), first=f)
            return self._retarget(f, n)
        elif name == "train_held_out":
            it, B, every, rows, rule = kw["iters"], kw["B"], kw["every"], kw["held_rows"], kw["rule"]
            smp = self.each if kw.get("each") else self.sampler
            if not twin:
                hits, loss, best, w = net.train_sampled_held_out(smp, it, B, st, mo, every, rows, rule)
            else:
                hits, loss, Ws = [], [], []
                for j in range(1, it + 1):
                    net.forget_lookahead(); net.gradient_step_indexed(smp.sample(B), st, mo)
                    if j % every == 0 or j == it:
                        net.forget_lookahead()
                        h, l = net.evaluate_range(0, rows, held_out=True)
                        hits.append(h); loss.append(l); Ws.append(net.get_weights())
                best = gnn.best_point(hits, loss, rule)
                w = Ws[best] if best >= 0 else None
            return {"curve_hits": np.array(hits, dtype=np.int64), "curve_loss": np.array(loss), "best": np.array(best), "best_W": w}
        elif name == "train_fgsm":
            p = s2.CLIP_ONLY
            if not twin:
                net.train_sampled_fgsm(self.sampler, kw["iters"], kw["B"], st, mo, p["eps"], p["clip"])
            else:
                for _ in range(kw["iters"]):
                    idx = self.sampler.sample(kw["B"])
                    net.forget_lookahead()
                    g = net.input_gradient(self.X[idx], self.Y[idx])
                    adv = ac.perturb(self.X[idx], g, p["eps"], p["clip"], dtype=np.float32).astype(np.float64)
                    net.forget_lookahead(); net.gradientStep(adv, st, mo, False, expected=self.Y[idx])
        elif name == "refused2":
            return self.refused2(kw, Xh, Yh)
        return {}


def _confusion2(labels, Y):
    d = Y.shape[1]
    conf = np.zeros((d, d), dtype=np.int64)
    for lab, e in zip(labels, s2.stc.expected_class(Y)):
        conf[e, lab] += 1
    return conf


def run_prefix2(gnn, oracle_mod, monkeypatch, tmp_path, case, n_ops=None):
    """run_prefix for a sequence of the second draw: the handle and its teacher T against their twins (bitwise) and Model2."""
    ops = case["ops"][:n_ops]
    bf16, dims = case["dtype"] == "bf16", case["dims"]
    Xh, Yh = sq.host_pool(case["seed"], dims[0], dims[-1])
    w0 = sq.start_weights(oracle_mod, dims)
    a = _Side2(gnn, _net(gnn, case), "a", str(tmp_path), False, case, lambda c, seed: _net(gnn, c, seed))
    b = _Side2(gnn, _twin(gnn, monkeypatch, case), "b", str(tmp_path), True, case, lambda c, seed: _twin(gnn, monkeypatch, c, seed))
    model = s2.Model2(oracle_mod, case, reads=not bf16)
    bud = _Budget()
    X, Y = sq.dataset(case["seed"], 0, dims[0], dims[-1])
    first_at = {}
    try:
        for s in (a, b):
            s.net.set_weights(w0); s.upload(X, Y); s.teacher(oracle_mod)
        split = lambda w, d=dims: np_oracle.split(w, d)
        fwd16 = lambda w, rows, d=dims: np_oracle.forward_bf16(split(w, d), rows, case["inner"], case["out_kind"], case["last"])[2]
        for i, (name, kw) in enumerate(ops):
            ctx = _ctx(case, ops, i)
            if name == "upload":
                X, Y = sq.dataset(case["seed"], kw["which"], dims[0], dims[-1])
                b.net.forget_lookahead()
                a.upload(X, Y); b.upload(X, Y)
                got = twin = {}
            else:
                got, twin = a.do(name, kw, Xh, Yh, i), b.do(name, kw, Xh, Yh, i)
            before_Y = model.Y
            want = model.apply(i, (name, kw))
            if not a.net.time == b.net.time == want["time"]:
                raise _Fail("time %d, the twin's %d, the model's %d\n%s" % (a.net.time, b.net.time, want["time"], ctx))
            if name == "teacher":
                if not a.T.net.time == b.T.net.time == want["Ttime"]:
                    raise _Fail("the teacher's time %d, its twin's %d, the model's %d\n%s" % (a.T.net.time, b.T.net.time, want["Ttime"], ctx))
                if kw["op"][0] == "get_weights":
                    got, twin = dict(got, TV=a.T.net.get_momentum()), dict(twin, TV=b.T.net.get_momentum())
                    want = dict(want, TV=model.teacher.V)
            for k in got:
                if got[k] is None or twin[k] is None:
                    if got[k] is not twin[k]: raise _Fail("%s: one side has none\n%s" % (k, ctx))
                else:
                    _same(got[k], twin[k], k, ctx)
            if name == "refused2" and int(got["code"]) != REFUSED2[kw["kind"]]:
                raise _Fail("the refused call returned %d\n%s" % (got["code"], ctx))
            Xs, Ys = (a.Xo, a.Yo) if kw.get("held") else (a.X, a.Y)
            if "confusion" in got:
                if not np.array_equal(got["confusion"], _confusion2(got["labels"], Ys[kw["first"]:kw["first"] + kw["n"]])):
                    raise _Fail("the confusion matrix is not the count of the returned labels\n%s" % ctx)
            if sq.is_checkpoint(i, ops):
                got = dict(got, W=a.net.get_weights(), V=a.net.get_momentum())
                _same(got["W"], b.net.get_weights(), "weights", ctx)
                _same(got["V"], b.net.get_momentum(), "momentum", ctx)
                want = dict(want, W=model.W, V=model.V)
            # what needs the weights of the moment (a sign, a gradient held to 2e-5 of its largest element): the TWIN's, read behind the op
            if "grad_in" in got or (name == "fgsm_range" and kw["signed"]):
                wt = b.net.get_weights()
                rows = (Xh[kw["off"]:kw["off"] + kw["n"]], Yh[kw["off"]:kw["off"] + kw["n"]]) if name == "input_gradient" else \
                       (Xs[kw["first"]:kw["first"] + kw["n"]], Ys[kw["first"]:kw["first"] + kw["n"]])
                ref = np.concatenate([model.input_gradient(rows[0][o:o + sq.MAX_BATCH], rows[1][o:o + sq.MAX_BATCH], W=wt)
                                      for o in range(0, kw["n"], sq.MAX_BATCH)])
                if "grad_in" in got:
                    err, budget = s2.igc.within(got["grad_in"], ref, bf16)
                    bud.check("input gradient", err, budget, ctx)
                else:
                    ok = ac.decided(ref, rows[0], case["inner"], bf16)
                    bud.check("undecided share", 1.0 - ok.mean(), ac.UNDECIDED_CAP, ctx)
                    adv = ac.perturb(rows[0], ref, s2.SIGNED["eps"], s2.SIGNED["clip"], dtype=np.float32).astype(np.float64)
                    if not np.array_equal(got["rows"][ok], adv[ok]):
                        raise _Fail("perturbed rows differ from the float32 formula on %d decided elements\n%s" % ((got["rows"][ok] != adv[ok]).sum(), ctx))
            if "rows" in got and not kw["signed"] and not np.array_equal(got["rows"], s2.clip_rows(Xs[kw["first"]:kw["first"] + kw["n"]])):
                raise _Fail("clipped rows differ from the formula\n%s" % ctx)
            if name == "distill":
                f, n, keep = kw["first"], kw["n"], kw["keep"]
                if bf16:                                             # the blend of the teacher's bf16 outputs on the weights ITS twin reports
                    t = {"self": lambda: fwd16(b.net.get_weights(), a.X[f:f + n]),
                         "other": lambda: fwd16(b.T.net.get_weights(), a.X[f:f + n], s2.teacher_case(case)["dims"]),
                         "group": lambda: np.mean([fwd16(w, a.X[f:f + n]) for w in a.group_W], axis=0)}[kw["teacher"]]()
                    blend = keep * before_Y[f:f + n] + (1.0 - keep) * t
                else:
                    blend = want["targets"]
                if keep == 1.0:
                    if not np.array_equal(got["targets"], before_Y[f:f + n]): raise _Fail("keep = 1 changed the targets\n%s" % ctx)
                else:
                    bud.check("distilled targets" + (" (bf16)" if bf16 else ""), np.abs(got["targets"] - blend).max(),
                              (sq.BF16_OUT if bf16 else sq.OUT_ATOL) * (1.0 - keep), ctx)
                model.set_device_targets(f, got["targets"])
            elif "targets" in got and not np.array_equal(got["targets"], want["targets"]):
                raise _Fail("the targets differ from the model's\n%s" % ctx)
            if "idx" in got and not np.array_equal(got["idx"], want["idx"]):
                raise _Fail("the sampler's draw differs from the oracle sampler's\n%s" % ctx)
            if not bf16:
                got = {k: v for k, v in got.items() if k not in ("grad_in", "targets")}
                if "best" in got:
                    if want["best_clear"] and int(got["best"]) != want["best"]:
                        raise _Fail("best point %d, the model's %d\n%s" % (got["best"], want["best"], ctx))
                    if int(got["best"]) != want["best"]: got.pop("best_W")
                    if np.any(np.abs(got["curve_hits"] - want["curve_hits"]) > want["curve_unsafe"]):
                        raise _Fail("held-out hits %r, the model's %r, unsafe rows %r\n%s" % (got["curve_hits"], want["curve_hits"], want["curve_unsafe"], ctx))
                for what, frac in s2.fractions(case, got, want, want["steps"]):
                    bud.check(what, frac, 1.0, ctx)
                if "labels" in got:
                    safe = want["safe"]
                    if not np.array_equal(got["labels"][safe], want["labels"][safe]):
                        raise _Fail("labels differ from the oracle's on %d safe rows\n%s" % ((got["labels"][safe] != want["labels"][safe]).sum(), ctx))
            else:
                if name == "propagate":
                    bud.check("outputs (bf16)", np.abs(got["out"] - fwd16(b.net.get_weights(), Xh[kw["off"]:kw["off"] + kw["n"]])).max(), sq.BF16_OUT, ctx)
                if name == "propagate_set":
                    bud.check("outputs (bf16)", np.abs(got["out"] - fwd16(b.net.get_weights(), Xs[kw["first"]:kw["first"] + kw["n"]])).max(), sq.BF16_OUT, ctx)
                n = want["steps"]
                if n in sq.BF16_W and n not in first_at:
                    first_at[n] = i
                    bud.check("weights after %d steps (bf16)" % n, np.abs(a.net.get_weights() - model.W).max(), sq.BF16_W[n], ctx)
                    bud.check("momentum after %d steps (bf16)" % n, np.abs(a.net.get_momentum() - model.V).max(), sq.BF16_W[n], ctx)
    finally:
        for s in (a, b):
            s.close()
    return bud.used


@pytest.mark.parametrize("i", range(s2.N_LONE), ids=[s2.lone_case(i)["id"] for i in range(s2.N_LONE)])
def test_lone_sequences_of_the_second_draw(gnn, oracle_mod, monkeypatch, tmp_path, i):
    if _forced_path():
        pytest.skip("path forced by the environment")
    case = s2.lone_case(i)
    used = run_prefix2(gnn, oracle_mod, monkeypatch, tmp_path, case)
    print("call-sequence %s (%d ops): largest fraction of each budget used: %s"
          % (case["id"], len(case["ops"]), "  ".join("%s %.3f" % (k, v) for k, v in sorted(used.items()))))


# ---- groups ---------------------------------------------------------------------------------------------------------------------
def _group(gnn, case):
    dt = gnn.DTYPE_BF16 if case["dtype"] == "bf16" else gnn.DTYPE_F32
    return gnn.NetGroup(case["dims"], case["wseeds"], out_kind=case["out_kind"], inner_act=case["inner"], last_act=case["last"], dtype=dt,
                        max_batch=sq.MAX_BATCH)


def run_group_prefix(gnn, oracle_mod, tmp_path, case, n_ops=None):
    """The first n_ops ops of a group sequence on a NetGroup, against K lone handles that make member k's calls with steps[k],
    momenta[k] and samplers[k] (bit for bit: time and every returned array after every op, weights and momentum every 8 ops and at
    the end) and, f32, the fp64 model of member 0 and of the last member."""
    ops = case["ops"][:n_ops]
    K, dims, bf16 = case["K"], case["dims"], case["dtype"] == "bf16"
    Xh, Yh = sq.host_pool(case["seed"], dims[0], dims[-1])
    Wnew, Vnew = sq.replacement_weights(oracle_mod, dims), sq.replacement_momentum(oracle_mod, dims)
    g = _group(gnn, case)
    grouped = g.launches_per_step == 2
    X, Y = sq.dataset(case["seed"], 0, dims[0], dims[-1])
    members, lones, models = [], [], {}
    for k in range(K):
        mc = sq.member_case(case, k)
        m = _Side(gnn, g.members[k], "g%d" % k, str(tmp_path), False, case["steps"][k], case["momenta"][k])
        l = _Side(gnn, _net(gnn, case, seed=case["wseeds"][k]), "l%d" % k, str(tmp_path), False, case["steps"][k], case["momenta"][k])
        w0 = sq.start_weights(oracle_mod, dims, seed=case["wseeds"][k])
        for s in (m, l):
            s.each_seed = case["each_seeds"][k]
            s.net.set_weights(w0)
        members.append(m); lones.append(l)
        if not bf16 and k in (0, K - 1):
            models[k] = sq.Model(oracle_mod, mc)
    g.upload_dataset(X, Y)
    for k in range(K):
        members[k].upload(X, Y, group=g); lones[k].upload(X, Y)
    shared = members[0].sampler                                    # the group's ONE sampler; every lone net has its own in the same state
    bud = _Budget()
    st, mo = case["steps"], case["momenta"]
    try:
        for i, (name, kw) in enumerate(ops):
            ctx = _ctx(case, ops, i)
            got = [{} for _ in range(K)]
            if name == "member":
                k, (mname, mkw) = kw["k"], kw["op"]
                mkw = dict(mkw, _W=Wnew, _V=Vnew) if mname in ("set_weights", "set_momentum") else mkw
                got[k] = members[k].do(mname, mkw, Xh, Yh, 1)
                if mname == "refused" and int(got[k].pop("code")) != 5:      # GNN_ERR_STATE: the group owns its data set
                    raise _Fail("the refused call did not return GNN_ERR_STATE\n%s" % ctx)
            elif name == "g_train_range":
                g.train_range(kw["first"], kw["B"], kw["n_steps"], st, mo)
            elif name == "g_train_sampled":
                smp = shared if kw["mode"] == "shared" else [m.each for m in members]
                g.train_sampled(smp, kw["iters"], kw["B"], st, mo)
                if kw["mode"] == "sizes" and g.sampled_each_iterations != ((kw["iters"], 0) if grouped and K > 1 else (0, kw["iters"])):
                    raise _Fail("sampled_each_iterations %r\n%s" % (g.sampled_each_iterations, ctx))
            elif name == "g_train_observed":
                val = g.train_sampled_observed(shared, kw["iters"], kw["B"], st, mo, kw["V"])
                got = [{"val": val[:, k].copy()} for k in range(K)]
            elif name == "g_evaluate":
                hits, loss, _ = g.evaluate_range(kw["first"], kw["n"])
                got = [{"hits": np.array(hits[k]), "loss_sum": np.array(loss[k])} for k in range(K)]
            elif name == "g_confusion":
                member, _, lab = g.confusion_range(kw["first"], kw["n"], labels=True)
                got = [{"confusion": member[k], "labels": lab[k]} for k in range(K)]
            elif name == "g_ensemble":
                mean = g.ensemble_propagate_range(kw["first"], kw["n"])
                rows = X[kw["first"]:kw["first"] + kw["n"]]
                ref = np.mean([l.net.propagate(rows) for l in lones], axis=0)
                bud.check("ensemble outputs", np.abs(mean - ref).max(), sq.BF16_OUT if bf16 else sq.OUT_ATOL, ctx)
            elif name == "g_upload":
                X, Y = sq.dataset(case["seed"], kw["which"], dims[0], dims[-1])
                g.upload_dataset(X, Y)
                for m in members:
                    m.upload(X, Y, group=g)
            for k in range(K):
                lop = sq.member_op((name, kw), k)
                if lop is None:
                    want = {}
                elif lop[0] == "upload":
                    lones[k].upload(X, Y); want = {}
                else:
                    lkw = dict(lop[1], _W=Wnew, _V=Vnew) if lop[0] in ("set_weights", "set_momentum") else lop[1]
                    want = lones[k].do(lop[0], lkw, Xh, Yh, 1)
                kctx = "member %d; %s" % (k, ctx)
                if members[k].net.time != lones[k].net.time:
                    raise _Fail("time %d, the lone net's %d\n%s" % (members[k].net.time, lones[k].net.time, kctx))
                for key in got[k]:
                    if key == "loss_sum" and name == "g_evaluate" and g.eval_launches == 2:
                        # the grouped forward launch (csrc/group_eval_kernel.h) adds the same f32 products in another order than the
                        # lone net's kernels: the header promises the lone net's DEFINITION of the sum, its bits only member after
                        # member -- the f32 summation-order bound (sequence_cases.order_bound)
                        bud.check("group loss sums against the lone nets' (order bound)", abs(got[k][key] - want[key]),
                                  sq.order_bound(want[key], kw["n"]), kctx)
                    elif key == "val" and g.observed_launches == 3:
                        # ... and so does the grouped validation launch (bits promised where gnn_mlp_group_observed_launches() is 0)
                        bud.check("group validation curves against the lone nets' (order bound)", np.abs(got[k][key] - want[key]),
                                  [sq.order_bound(v * kw["V"], kw["V"]) / kw["V"] for v in want[key]], kctx)
                    elif key in ("val", "loss_sum"):
                        if not np.all(np.abs(got[k][key] - want[key]) <= 1e-12 * np.abs(want[key])):
                            raise _Fail("%s differs from the lone net's by %.3g relative\n%s" % (key, np.abs(got[k][key] / want[key] - 1).max(), kctx))
                    else:
                        _same(got[k][key], want[key], key, kctx)
                if sq.is_checkpoint(i, ops):
                    got[k] = dict(got[k], W=members[k].net.get_weights(), V=members[k].net.get_momentum())
                    _same(got[k]["W"], lones[k].net.get_weights(), "weights", kctx)
                    _same(got[k]["V"], lones[k].net.get_momentum(), "momentum", kctx)
                if k in models:
                    mwant = models[k].apply(i, lop) if lop is not None else {"time": models[k].time, "steps": models[k].steps}
                    if members[k].net.time != mwant["time"]:
                        raise _Fail("time %d, the model's %d\n%s" % (members[k].net.time, mwant["time"], kctx))
                    if "W" in got[k]:
                        mwant = dict(mwant, W=models[k].W, V=models[k].V)
                    _against_model(bud, case, name, got[k], mwant, mwant["steps"], kctx)
    finally:
        for l in lones:
            l.close()
        for m in members:
            for x in (m.sampler, m.each):
                if x is not None: x.close()
        g.close()
    return bud.used


def run_group_prefix2(gnn, oracle_mod, tmp_path, case, n_ops=None):
    """run_group_prefix for a group sequence of the second draw: the NetGroup against K lone handles that make member k's calls
    (bit for bit, but loss sums of grouped evaluation launches: the order bound) and, f32, Model2 of member 0 and of the last."""
    ops = case["ops"][:n_ops]
    K, dims, bf16 = case["K"], case["dims"], case["dtype"] == "bf16"
    Xh, Yh = sq.host_pool(case["seed"], dims[0], dims[-1])
    g = _group(gnn, case)
    X, Y = sq.dataset(case["seed"], 0, dims[0], dims[-1])
    members, lones, models = [], [], {}
    for k in range(K):
        mc = s2.member_case(case, k)
        m = _Side2(gnn, g.members[k], "g%d" % k, str(tmp_path), False, mc, None)
        l = _Side2(gnn, _net(gnn, case, seed=case["wseeds"][k]), "l%d" % k, str(tmp_path), False, mc, None)
        w0 = sq.start_weights(oracle_mod, dims, seed=case["wseeds"][k])
        for s in (m, l):
            s.each_seed, s.step, s.mom = case["each_seeds"][k], case["steps"][k], case["momenta"][k]
            s.net.set_weights(w0)
        members.append(m); lones.append(l)
        if not bf16 and k in (0, K - 1):
            models[k] = s2.Model2(oracle_mod, mc, with_teacher=False)
    g.upload_dataset(X, Y)
    for k in range(K):
        members[k].upload(X, Y, group=g); lones[k].upload(X, Y)
    shared = members[0].sampler
    bud = _Budget()
    st, mo = case["steps"], case["momenta"]
    order = g.eval_launches == 2                                  # the grouped forward launch adds in another order than the lone nets'
    try:
        for i, (name, kw) in enumerate(ops):
            ctx = _ctx(case, ops, i)
            got = [{} for _ in range(K)]
            if name == "member":
                got[kw["k"]] = members[kw["k"]].do(kw["op"][0], kw["op"][1], Xh, Yh, 1)
            elif name == "g_train_range":
                g.train_range(kw["first"], kw["B"], kw["n_steps"], st, mo)
            elif name == "g_train_sampled":
                g.train_sampled(shared if kw["mode"] == "shared" else [m.each for m in members], kw["iters"], kw["B"], st, mo)
            elif name == "g_set_targets":
                g.set_targets(s2.target_rows(case["seed"], kw["tseed"], kw["n"], dims[-1]), first=kw["first"])
                for m in members:
                    m._retarget(kw["first"], kw["n"])
            elif name == "g_upload_held_out":
                Xo, Yo = s2.held_set(case["seed"], kw["size"], dims[0], dims[-1])
                g.upload_held_out(Xo, Yo)
                for m in members:
                    m.Xo, m.Yo = Xo, Yo
            elif name == "g_evaluate_set":
                hits, loss, _ = g.evaluate_range(kw["first"], kw["n"], held_out=kw["held"])
                got = [{"hits": np.array(hits[k]), "loss_sum": np.array(loss[k])} for k in range(K)]
            elif name == "g_confusion_set":
                member, _, lab = g.confusion_range(kw["first"], kw["n"], labels=True, held_out=kw["held"])
                got = [{"confusion": member[k], "labels": lab[k]} for k in range(K)]
            elif name == "g_ensemble_set":
                mean = g.ensemble_propagate_range(kw["first"], kw["n"], held_out=kw["held"])
                ref = np.mean([l.net.propagate_range(kw["first"], kw["n"], held_out=kw["held"]) for l in lones], axis=0)
                bud.check("ensemble outputs", np.abs(mean - ref).max(), sq.BF16_OUT if bf16 else sq.OUT_ATOL, ctx)
            elif name == "g_input_gradient":
                mem, ens = g.input_gradient_range(kw["first"], kw["n"], members=True)
                got = [{"grad_in": mem[k]} for k in range(K)]
                acc = mem[0].astype(np.float32)
                for k in range(1, K):
                    acc = acc + mem[k].astype(np.float32)
                _same(ens, (acc / np.float32(K)).astype(np.float64), "the ensemble's input gradient (f32 mean in member order)", ctx)
            elif name == "g_train_held_out":
                hits, loss, _, best, w = g.train_sampled_held_out([m.each for m in members], kw["iters"], kw["B"], st, mo, kw["every"],
                                                                  kw["held_rows"], kw["rule"])
                got = [{"curve_hits": hits[:, k].copy(), "curve_loss": loss[:, k].copy(), "best": np.array(best[k]), "best_W": w[k].copy()}
                       for k in range(K)]
            for k in range(K):
                lop = s2.member_op((name, kw), k)
                if lop is None:
                    want = {}
                elif lop[0] in ("set_weights", "set_momentum"):
                    raise ValueError(lop[0])
                else:
                    want = lones[k].do(lop[0], lop[1], Xh, Yh, 1)
                kctx = "member %d; %s" % (k, ctx)
                if members[k].net.time != lones[k].net.time:
                    raise _Fail("time %d, the lone net's %d\n%s" % (members[k].net.time, lones[k].net.time, kctx))
                if "best" in got[k] and order:
                    # a decision between two points whose losses lie within the order bound of each other is either net's
                    l = want["curve_loss"]
                    gap = min([abs(l[p] - l[q]) for p in range(len(l)) for q in range(p)] or [np.inf])
                    if gap <= 2 * sq.order_bound(np.abs(l).max(), kw["held_rows"]) and int(got[k]["best"]) != int(want["best"]):
                        got[k].pop("best"); got[k].pop("best_W")
                for key in got[k]:
                    if key in ("loss_sum", "curve_loss") and order and name != "member":
                        rows = kw["n"] if key == "loss_sum" else kw["held_rows"]
                        bud.check("group loss sums against the lone nets' (order bound)", np.abs(got[k][key] - want[key]),
                                  [sq.order_bound(v, rows) for v in np.atleast_1d(want[key])], kctx)
                    elif key in ("loss_sum", "curve_loss"):
                        if not np.all(np.abs(got[k][key] - want[key]) <= 1e-12 * np.abs(want[key])):
                            raise _Fail("%s differs from the lone net's by %.3g relative\n%s" % (key, np.abs(got[k][key] / want[key] - 1).max(), kctx))
                    else:
                        _same(got[k][key], want[key], key, kctx)
                if "confusion" in got[k]:
                    Ys = members[k].Yo if kw["held"] else members[k].Y
                    if not np.array_equal(got[k]["confusion"], _confusion2(got[k]["labels"], Ys[kw["first"]:kw["first"] + kw["n"]])):
                        raise _Fail("the confusion matrix is not the count of the returned labels\n%s" % kctx)
                if sq.is_checkpoint(i, ops):
                    got[k] = dict(got[k], W=members[k].net.get_weights(), V=members[k].net.get_momentum())
                    _same(got[k]["W"], lones[k].net.get_weights(), "weights", kctx)
                    _same(got[k]["V"], lones[k].net.get_momentum(), "momentum", kctx)
                if k in models:
                    mw = models[k].apply(i, lop) if lop is not None else {"time": models[k].time, "steps": models[k].steps}
                    if members[k].net.time != mw["time"]:
                        raise _Fail("time %d, the model's %d\n%s" % (members[k].net.time, mw["time"], kctx))
                    if "W" in got[k]:
                        mw = dict(mw, W=models[k].W, V=models[k].V)
                    gk = dict(got[k])
                    if "grad_in" in gk:                               # (held to 2e-5 of its largest element: on the lone net's weights of the moment)
                        rows = slice(lop[1]["first"], lop[1]["first"] + lop[1]["n"])
                        wl = lones[k].net.get_weights()
                        ref = np.concatenate([models[k].input_gradient(members[k].X[rows][o:o + sq.MAX_BATCH], members[k].Y[rows][o:o + sq.MAX_BATCH], W=wl)
                                              for o in range(0, lop[1]["n"], sq.MAX_BATCH)])
                        err, budget = s2.igc.within(gk.pop("grad_in"), ref, False)
                        bud.check("input gradient", err, budget, kctx)
                    if "targets" in gk and not np.array_equal(gk.pop("targets"), mw["targets"]):
                        raise _Fail("the targets differ from the model's\n%s" % kctx)
                    if "best" in gk and int(gk["best"]) != mw["best"]:
                        if mw["best_clear"]: raise _Fail("best point %d, the model's %d\n%s" % (gk["best"], mw["best"], kctx))
                        gk.pop("best_W")
                    if "curve_hits" in gk and np.any(np.abs(gk["curve_hits"] - mw["curve_hits"]) > mw["curve_unsafe"]):
                        raise _Fail("held-out hits %r, the model's %r\n%s" % (gk["curve_hits"], mw["curve_hits"], kctx))
                    for what, frac in s2.fractions(case, gk, mw, mw["steps"]):
                        bud.check(what, frac, 1.0, kctx)
                    if "labels" in gk and not np.array_equal(gk["labels"][mw["safe"]], mw["labels"][mw["safe"]]):
                        raise _Fail("labels differ from the oracle's on safe rows\n%s" % kctx)
    finally:
        for l in lones:
            l.close()
        for m in members:
            for x in (m.sampler, m.each):
                if x is not None: x.close()
        g.close()
    return bud.used


@pytest.mark.parametrize("i", range(s2.N_GROUP), ids=[s2.group_case(i)["id"] for i in range(s2.N_GROUP)])
def test_group_sequences_of_the_second_draw(gnn, oracle_mod, tmp_path, i):
    if _forced_path():
        pytest.skip("path forced by the environment")
    case = s2.group_case(i)
    used = run_group_prefix2(gnn, oracle_mod, tmp_path, case)
    print("call-sequence %s (%d ops, K = %d): largest fraction of each budget used: %s"
          % (case["id"], len(case["ops"]), case["K"], "  ".join("%s %.3f" % (k, v) for k, v in sorted(used.items()))))


@pytest.mark.parametrize("i", range(sq.N_GROUP), ids=[sq.group_case(i)["id"] for i in range(sq.N_GROUP)])
def test_group_sequences(gnn, oracle_mod, tmp_path, i):
    if _forced_path():
        pytest.skip("path forced by the environment")
    case = sq.group_case(i)
    used = run_group_prefix(gnn, oracle_mod, tmp_path, case)
    print("call-sequence %s (%d ops, K = %d): largest fraction of each budget used: %s"
          % (case["id"], len(case["ops"]), case["K"], "  ".join("%s %.3f" % (k, v) for k, v in sorted(used.items()))))


def test_the_groups_run_on_the_launches_they_are_for(gnn):
    if _forced_path():
        pytest.skip("path forced by the environment")
    per_step = {}
    for i in range(0, sq.N_GROUP, sq.SEEDS_PER_NET):
        case = sq.group_case(i)
        g = _group(gnn, case)
        per_step[case["net"]] = (g.launches_per_step, g.members[0].step_launches, case["dtype"], case["K"])
        g.close()
    assert per_step["g-f32-k2"][:2] == (2, 2) and per_step["g-f32-prebuilt-k3"][:2] == (2, 2), per_step
    assert per_step["g-bf16-k3"][0] == 2, per_step
    assert per_step["g-f32-off-path-k16"][0] == 0, per_step
    assert sorted(p[3] for p in per_step.values()) == [2, 3, 3, 16]
