"""Fixtures of the distillation tests (tests/test_distill_gpu.py runs them on the device, tests/test_distill_cpu.py shows on the
fp64 oracle that they discriminate): teachers, a student of another hidden shape, their resident rows, and numpy models of the
blend -- the right one in fp64 and in float32, and the wrong implementations the device tests must be able to see.  No GPU code.

ROWS.  N = 300 resident rows; every call works on the middle range [FIRST, FIRST + COUNT) = [37, 237), so that both neighbours
of the range are checked as untouched.  Handles are made with blocks of BLOCK = 64 rows (max_batch = 64 and
GNN_MLP_EVAL_ROWS=0, as tests/test_group_eval_gpu.py shrinks them): the range is three full blocks and a ragged one of 8 rows.
Inputs as tests/group_eval_cases.py draws them -- centred, half the entries exactly zero -- f32-exact.

NETS.  Weights are the f32-rounded Random(seed) draw times the case's scale (group_eval_cases.member_weights).
  D10  teachers 24-16-12-10 softmax / leaky ReLU, K = 3: passes the group evaluation plan (eval_launches == 2); student 24-14-10.
       10 outputs in rows of stride 16: the blend kernel's scalar form, six padding columns.
  D20  teachers 24-16-20 General tanh / sigmoid, K = 3: 20 outputs, outside the plan (member after member, eval_launches == 0);
       student 24-12-20.  Rows of stride 32: the kernel's 16-byte form, twelve padding columns.

The scale of D10 is 1.0 because at 1.5 the bf16 ORACLE's outputs already lie 0.0070 from the fp64 oracle's, outside the bf16
output budget of 5e-3 (at 1.0: 0.0020); tests/group_eval_cases.py lowered its bf16 scales for the same reason.

BOUNDS.  keep = 0 and keep = 1 are exact.  keep = 0.25: 2^-22 absolute against the fp64 blend of the two read-back f32 arrays --
three f32 roundings (two products, one sum) of at most 2^-25 each on values in [0, 1], with margin.  Outputs against the fp64
oracle: 2e-4 (f32) and 5e-3 (bf16), the budgets of tests/test_group_eval_gpu.py."""
import numpy as np

from tests import np_oracle

LEAKY, SIGMOID, TANH, RELU, IDENT = range(5)
SCE, GENERAL = 0, 1
F32, BF16 = 0, 1
N, FIRST, COUNT, BLOCK = 300, 37, 200, 64
K = 3
KEEP = 0.25
BLEND_BOUND = 2.0 ** -22
OUT_BOUND = {F32: 2e-4, BF16: 5e-3}
ROW_GAP = 2.0 ** -12          # any two rows of the range differ by this much in some class of the teacher's output
STUDENT_SEED = 7


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


class Case:
    def __init__(self, name, teacher, student, kind, inner, last, scale, grouped):
        self.name, self.teacher, self.student, self.kind, self.inner, self.last = name, teacher, student, kind, inner, last
        self.scale, self.grouped = scale, grouped
        self.d_out = teacher[-1]
        self.ld = (self.d_out + 15) // 16 * 16      # the stride of a resident expected row

    def __repr__(self):
        return self.name


CASES = {
    "D10": Case("D10", [24, 16, 12, 10], [24, 14, 10], SCE, LEAKY, IDENT, 1.0, True),
    "D20": Case("D20", [24, 16, 20], [24, 12, 20], GENERAL, TANH, SIGMOID, 1.0, False),
}
_cache = {}


def _once(key, make):
    if key not in _cache:
        v = make()
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        _cache[key] = v
    return _cache[key]


def inputs(case):
    def make():
        rng = np.random.default_rng(5100 + case.d_out)
        return f32(rng.standard_normal((N, case.teacher[0])) * (rng.random((N, case.teacher[0])) < 0.5))
    return _once((case.name, "X"), make)


def labels(case):
    return _once((case.name, "labels"), lambda: np.random.default_rng(5200 + case.d_out).integers(0, case.d_out, N))


def onehot(case):
    return _once((case.name, "Y"), lambda: np.eye(case.d_out)[labels(case)])


def draw(oracle_mod, case, dims, seed):
    """The f32-rounded Random(seed) draw (SCE:139-156) times the case's scale, as an f32 net holds it: flat, f32-exact."""
    def make():
        net = oracle_mod.OracleNet(dims, out_kind=case.kind, inner_act=case.inner, last_act=case.last, seed=seed)
        w = f32(f32(net.get_weights()) * case.scale)
        net.close()
        return w
    return _once((case.name, tuple(dims), seed), make)


def teacher_weights(oracle_mod, case, k):
    return draw(oracle_mod, case, case.teacher, k + 1)


def student_weights(oracle_mod, case):
    return draw(oracle_mod, case, case.student, STUDENT_SEED)


def outputs(case, dims, w, X, dtype):
    """propagate() of rows X in fp64 (np_oracle.forward), or its bf16 form."""
    Ws = np_oracle.split(np.asarray(w, dtype=np.float64), dims)
    if dtype == BF16:
        return np_oracle.forward_bf16(Ws, X, case.inner, case.kind, case.last)[2]
    return np_oracle.forward(Ws, X, case.inner, case.kind, case.last)[1]


def teacher_outputs(oracle_mod, case, dtype):
    """[K][N][d_out]: every teacher's outputs on the resident rows -- computed once, shared, read-only."""
    return _once((case.name, "teachers", dtype), lambda: np.stack(
        [outputs(case, case.teacher, teacher_weights(oracle_mod, case, k), inputs(case), dtype) for k in range(K)]))


def ensemble_f32(outs, k_div=None):
    """The mean as group_combine_kernel forms it from f32 member rows: an f32 sum in member order, one division by (float)K."""
    o = np.asarray(outs).astype(np.float32)
    s = o[0].copy()
    for k in range(1, o.shape[0]):
        s = (s + o[k]).astype(np.float32)
    return (s / np.float32(o.shape[0] if k_div is None else k_div)).astype(np.float32).astype(np.float64)


def blend_f64(y, t, keep):
    return keep * np.asarray(y, dtype=np.float64) + (1.0 - keep) * np.asarray(t, dtype=np.float64)


def blend_f32(y, t, keep):
    """The kernel's arithmetic restated: keep_f * y + (1.f - keep_f) * t, every product and the sum rounded to float32."""
    f = np.float32
    k = f(keep)
    a = (k * np.asarray(y).astype(f)).astype(f)
    b = ((f(1.0) - k).astype(f) * np.asarray(t).astype(f)).astype(f)
    return (a + b).astype(f).astype(np.float64)


def distilled(case, y_all, t_range, keep, blend=blend_f64):
    """The resident expected rows [N][d_out] after the right call: the range blended, every other row as it was."""
    y = np.array(y_all, dtype=np.float64)
    y[FIRST:FIRST + COUNT] = blend(y[FIRST:FIRST + COUNT], t_range, keep)
    return y


# ---- wrong implementations: what a device with the fault would leave in rows [0, N) ----------------------------------------
def wrong_block_offset(case, y_all, t_all, keep):
    """Every block after the first reads the teacher rows of the block before it (a row offset wrong by one block)."""
    r = np.arange(COUNT)
    src = FIRST + np.where(r >= BLOCK, r - BLOCK, r)
    return distilled(case, y_all, t_all[src], keep)


def wrong_dense_stride(case, y_all, t_all, keep):
    """The expected rows addressed with the dense stride d_out in place of ld: element (r, c) of the range is read and written
    at word r * d_out + c of the padded image that starts at row FIRST."""
    d, ld = case.d_out, case.ld
    img = np.zeros((N + 16, ld))
    img[:N, :d] = y_all
    flat = img.reshape(-1)
    base = FIRST * ld
    idx = base + np.arange(COUNT * d)
    flat[idx] = blend_f64(flat[idx], t_all[FIRST:FIRST + COUNT].reshape(-1), keep)
    return img[:N, :d].copy()


def wrong_k(case, y_all, outs_range, keep):
    """The members' sum divided by K + 1."""
    return distilled(case, y_all, ensemble_f32(outs_range, k_div=K + 1), keep)


def wrong_swapped(case, y_all, t_all, keep):
    """keep and 1 - keep swapped."""
    return distilled(case, y_all, t_all[FIRST:FIRST + COUNT], 1.0 - keep)


def oracle_sampled_run(oracle_mod, case, dtype, w, X, Y, iterations, batch, step, momentum, seed=1):
    """(w, v) of the student after train_sampled (NNT:82-90): the oracle stepping on the draws of the reference's sampler."""
    smp = oracle_mod.Sampler(len(X), seed=seed)
    w, v = np.array(w, dtype=np.float64), np.zeros(len(w))
    stepper = np_oracle.gradient_step_bf16 if dtype == BF16 else np_oracle.gradient_step
    for _ in range(iterations):
        idx = np.asarray(smp.sample(batch))
        w, v = stepper(w, v, case.student, X[idx], Y[idx], step, momentum, case.inner, case.kind, case.last)
    return w, v
