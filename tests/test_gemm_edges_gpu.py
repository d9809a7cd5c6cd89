"""The per-layer GEMM path (GNN_MLP_PATH=generic; bf16 inference and bf16 nets off the two-launch path; evaluation blocks
of 2 048 rows and more) at its ragged edges, against the fp64 matrix-form oracle (tests/np_oracle.py, pinned to the C oracle
by tests/test_oracle.py).

launch_gemm (csrc/launch_gemm.hip) and launch_gemm_bf16 (csrc/launch_bf16.hip) pick one of ~15 kernel forms per product from
M, N and K.  Each form can go wrong at three places that whole-tile shapes never reach: the guarded loads of a tile that is not
`interior`, a last K tile shorter than the form's BK (in bf16 down to half of one MFMA's K of 32), and the epilogue that stores
zeros past m_true / n_true and leaves the masters' padding alone.  Every row of TABLE is one net, one dtype and one batch size
chosen (by the tile choice of the two launchers) to send its products through the forms named in its comment with those
edges live; every row is checked for
  a. the forward pass, every probability (softmax) or output element (General);
  b. every element of every layer's exported gradient (EPI_STORE);
  c. weights and momentum after three fused steps (EPI_SGD) on host batches;
  d. the same three steps on device-resident rows whose successors in the data set (the rows the padded batch reads past B)
     hold values of 1e3: the bits of (c) -- those rows only ever meet exact zeros -- and so the oracle as well;
and the rows that reach an LDS-DMA form, with its masked epilogue, also against the register-staged kernels (bf16: bit for bit).
Tolerances are the suite's (test_random_shapes_gpu.py, test_bf16_gpu.py).

Hidden layers of ~1 000 units and more use smooth activations: a leaky-ReLU / ReLU unit within an f32 rounding of its kink
(one in a few million pre-activations) flips its derivative between the GPU's summation order and the oracle's, which moves
a whole rank-one slice of the gradient; the kinked activations run on the narrow nets, where that cannot happen.
"""
import os

import numpy as np
import pytest

from tests import np_oracle

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1
LEAKY, SIGMOID, TANH, RELU, IDENT = range(5)
SCE, GEN = "sce", "general"
STEP, MOMENTUM = 0.0125, 0.9
TOL = {  # probabilities / outputs, gradients (x max |G| of the layer), W and V after the steps
    F32: dict(p=2e-4, g=3e-5, g_abs=1e-9, w=3 * 2e-6),
    BF16: dict(p=5e-3, g=4e-3, g_abs=1e-7, w=2e-4),
}

# (dtype, class, dims, B, inner activation, environment switches, also bitwise against the non-DMA kernels): the comment names
# the forms (gemm_f32_kernel<BM, BN, .., WM> "f32 BMxBN", gemm_bf16_kernel<.., NSTG, WM> "reg", gemm_bf16_dma_kernel<.., NIMG>
# "DMA") and the edges the row is for.  M = pad_up(B), N and K the layer widths padded to 16.
TABLE = [
    # M 1024, N 2048 / 64: DMA 64x64 forward and backward data with m_true < M and n_true < N; wave-K logits (STORE), last-layer
    # gradient; the gradient's 64x64 stand-in for 256 tiles of 128 (2048 x 2048, SGD); 64x64 (eight waves) for 512 tiles
    (F32, SCE, [1020, 2040, 2040, 60], 1020, TANH, {}, True),
    # DMA 64x64 with two images (K 1024) and three (K 2048), DMA 32x32 logits and last gradient, all masked; reg 64x64 NSTG 5
    # backward data with K = 64, one half-filled K tile of 128
    (BF16, SCE, [1020, 2040, 2040, 60], 1020, TANH, {}, True),
    # f32 128x128 forward and backward data on whole tiles, masked in M and N; DMA 64x64; wave-K logits and gradient
    (F32, SCE, [2040, 2040, 1020, 60], 2040, SIGMOID, {}, True),
    # DMA 128x128 forward and backward data, masked; DMA 64x64 with three images; DMA 32x32
    (BF16, SCE, [2040, 2040, 1020, 60], 2040, SIGMOID, {}, True),
    # wave-K (whole) for every forward, backward-data and the last gradient product; 64x32 gradient
    (F32, SCE, [1020, 1020, 1020, 500], 500, IDENT, {}, False),
    # GNN_MLP_WAVEK=0: the same products on 32x32 tiles, masked
    (F32, SCE, [1020, 1020, 1020, 500], 500, IDENT, {"GNN_MLP_WAVEK": "0"}, False),
    # DMA 32x64 forward, DMA 32x32 logits, DMA 64x64 backward data, masked; gemm_bf16_group_kernel for all three gradients
    (BF16, SCE, [1020, 1020, 1020, 500], 500, IDENT, {}, True),
    # General: f32 128x128 forward and backward data ragged in M (4000 = 31 x 128 + 32), N (1504) and K (1008 = 31 x 32 + 16);
    # 64x64 forward, 64x64 backward data with K 48 < BK; 32x32 logits; 64x32 and ragged wave-K gradients; 32x32
    (F32, GEN, [1000, 1500, 600, 40], 3990, SIGMOID, {}, False),
    # General: reg 128x128 ragged in M, N and K (1008 = 15 x 64 + 48: a last tile of 32 + 16); reg 64x64 NSTG 5; reg 32x32
    # NSTG 5 logits; GNN_MLP_BF16_GROUP=0: the per-layer gradients the grouped launch would take (reg 64x64 NSTG 5, 32x32 NSTG 2)
    (BF16, GEN, [1000, 1500, 600, 40], 3990, SIGMOID, {"GNN_MLP_BF16_GROUP": "0"}, False),
    # f32 128x128 gradient + update (512 tiles of 128; ragged M 4000 and N 2000); 64x64 forward ragged in M; 32x32 logits
    (F32, SCE, [4000, 2000, 40], 600, TANH, {}, False),
    # reg 64x64 NSTG 2 gradient + update (2 016 tiles of 64, ragged); reg 64x64 NSTG 5 forward
    (BF16, SCE, [4000, 2000, 40], 600, TANH, {}, False),
    # the gradient's 64x64 stand-in for 256 tiles of 128, ragged in M, N (2000) and K (208 = 3 x 64 + 16); 32x32 elsewhere
    (F32, SCE, [2000, 2000, 30], 200, SIGMOID, {}, False),
    # reg 64x64 NSTG 5 ragged (forward, backward data with K 32, gradient); reg 32x32 NSTG 5 logits, NSTG 2 gradient
    (BF16, SCE, [2000, 2000, 30], 200, SIGMOID, {}, False),
    # B = 593 (1 mod 16): 32x32 forward (N 1040); wave-K with K 1040 (a K tail of 16); 64x32 gradient; 32x32 elsewhere
    (F32, SCE, [520, 1030, 1010, 100], 593, TANH, {}, False),
    # GNN_MLP_PATH=nomid4 (the per-layer middle between the one-launch first layer and gradient, as for nets whose middle
    # weights do not fit LDS): the forward's first layer over 608 rows is the RAGGED wave-K form (N 1040, K 528)
    (F32, SCE, [520, 1030, 1010, 100], 593, TANH, {"GNN_MLP_PATH": "nomid4"}, False),
    # reg 32x64 NSTG 5 forward with K 528 (a last tile of 16 = half an MFMA's K); reg 64x64; reg 32x32
    (BF16, SCE, [520, 1030, 1010, 100], 593, TANH, {}, False),
    # B = 1, dims 15 and 1 (mod 16): 32x32 forward with M 16; gradients with K = 16 (64x64 tiles, BK 64)
    (F32, SCE, [2047, 1023, 17], 1, LEAKY, {}, False),
    (BF16, SCE, [2047, 1023, 17], 1, LEAKY, {}, False),
    # everything on 32x32 tiles (bf16: NSTG 5 forward, NSTG 2 backward data, grouped gradients)
    (F32, SCE, [300, 70, 33, 17], 1, RELU, {}, False),
    (BF16, SCE, [300, 70, 33, 17], 1, RELU, {}, False),
    # B = 33; GNN_MLP_TAIL=0: logits of 15 outputs through the GEMM's STORE epilogue (K 48) instead of tail_kernel
    (F32, SCE, [300, 70, 33, 15], 33, LEAKY, {"GNN_MLP_TAIL": "0"}, False),
    (BF16, SCE, [300, 70, 33, 15], 33, LEAKY, {"GNN_MLP_TAIL": "0"}, False),
]


def _row_id(row):
    dt, cls, dims, B, act, env, _ = row
    sw = "".join("-" + k[len("GNN_MLP_"):].lower() + v for k, v in sorted(env.items()))
    return "%s-%s-%s-B%d%s" % ("f32" if dt == F32 else "bf16", cls, "-".join(map(str, dims)), B, sw)


def _pad16(n):
    return (n + 15) // 16 * 16


def _switches(env):
    return dict({"GNN_MLP_PATH": "generic"}, **env)


def _skip_if_forced(env):
    for k, v in _switches(env).items():
        if os.environ.get(k, v) != v:
            pytest.skip("%s forced by the environment" % k)


def _make(gnn, monkeypatch, dt, cls, dims, B, inner, env):
    """A handle on the per-layer GEMM path with the row's switches (read at create time only)."""
    with monkeypatch.context() as m:
        for k, v in _switches(env).items():
            m.setenv(k, v)
        if cls == SCE:
            return gnn.SoftmaxCrossEntropyNeuralNet(dims, inner_act=inner, dtype=dt, max_batch=B)
        return gnn.GeneralNeuralNet(dims, inner_act=inner, last_act=SIGMOID, dtype=dt, max_batch=B)


def _scaled_weights(net, dims, gain=2.0):
    """The Random(1) draws (U[-0.5, 0.5)), each layer scaled to a standard deviation of gain / sqrt(fan-in): pre-activations
    of order one at every width, so that softmax and sigmoid stay off saturation and f32 logit errors stay small."""
    w = net.get_weights()
    off = 0
    for l in range(len(dims) - 1):
        n = dims[l] * dims[l + 1]
        w[off:off + n] *= gain / (np.sqrt(dims[l]) * np.sqrt(1.0 / 12))
        off += n
    return w


def _oracle(dt, cls, inner):
    out_kind = 0 if cls == SCE else 1
    if dt == BF16:
        return (lambda Ws, X: np_oracle.forward_bf16(Ws, X, inner, out_kind, SIGMOID)[2],
                lambda Ws, X, Y: np_oracle.gradient_bf16(Ws, X, Y, inner, out_kind, SIGMOID),
                lambda w, v, dims, X, Y: np_oracle.gradient_step_bf16(w, v, dims, X, Y, STEP, MOMENTUM, inner, out_kind, SIGMOID))
    return (lambda Ws, X: np_oracle.forward(Ws, X, inner, out_kind, SIGMOID)[1],
            lambda Ws, X, Y: np_oracle.gradient(Ws, X, Y, inner, out_kind, SIGMOID),
            lambda w, v, dims, X, Y: np_oracle.gradient_step(w, v, dims, X, Y, STEP, MOMENTUM, inner, out_kind, SIGMOID))


def _assert_gradient(g, gref, dims, tol, what):
    off = 0
    for l in range(len(dims) - 1):
        n = dims[l] * dims[l + 1]
        ref_l = gref[off:off + n].reshape(dims[l], dims[l + 1]); off += n
        err = np.abs(g[l] - ref_l).max()
        assert err <= tol["g"] * np.abs(ref_l).max() + tol["g_abs"], (what, "layer %d" % l, err, np.abs(ref_l).max())


@pytest.mark.parametrize("row", TABLE, ids=[_row_id(r) for r in TABLE])
def test_per_layer_gemm_edges_against_oracle(gnn, monkeypatch, row):
    dt, cls, dims, B, inner, env, dma = row
    _skip_if_forced(env)
    assert _pad16(B) > B   # (d: the padded batch reads past B)
    tol = TOL[dt]
    fwd, grad, step = _oracle(dt, cls, inner)
    rng = np.random.default_rng(B * 7 + len(dims))
    X = rng.random((B, dims[0])) * (rng.random((B, dims[0])) < 0.5)
    Y = np.eye(dims[-1])[rng.integers(0, dims[-1], B)]
    X32 = X.astype(np.float32).astype(np.float64)   # inputs are f32 in HBM
    net = _make(gnn, monkeypatch, dt, cls, dims, B, inner, env)
    if _switches(env)["GNN_MLP_PATH"] == "generic":
        assert net.step_launches == 0, net.plan_note
    net.set_weights(_scaled_weights(net, dims))
    w0 = net.get_weights()                           # (the f32 masters)
    Ws = np_oracle.split(w0, dims)

    # a. forward, every element
    p = net.propagate(X)
    pref = fwd(Ws, X32)
    assert np.abs(p - pref).max() <= tol["p"], np.abs(p - pref).max()
    # b. every element of every layer's gradient (EPI_STORE)
    g = net.calculateWeightGradient(X, Y)
    _assert_gradient(g, grad(Ws, X32, Y), dims, tol, "gradient")
    # c. three fused steps (EPI_SGD) on host batches
    w, v = w0.copy(), np.zeros_like(w0)
    for s in range(3):
        net.gradientStep(X, STEP, MOMENTUM, False, expected=Y)
        w, v = step(w, v, dims, X32, Y)
    assert np.abs(net.get_weights() - w).max() <= tol["w"], np.abs(net.get_weights() - w).max()
    assert np.abs(net.get_momentum() - v).max() <= tol["w"], np.abs(net.get_momentum() - v).max()

    # d. the same steps on device-resident rows: rows B .. pad_up(B) - 1 of the A operand are the data set's next samples
    #    (large, finite: they meet the zeros of delta's padding rows, and 0 x NaN would be NaN)
    extra = _pad16(B) - B + 16
    Xd = np.vstack([X, 1e3 * (0.5 + rng.random((extra, dims[0])))])
    Yd = np.vstack([Y, np.eye(dims[-1])[rng.integers(0, dims[-1], extra)]])
    res = _make(gnn, monkeypatch, dt, cls, dims, B, inner, env)
    res.set_weights(w0)
    res.upload_dataset(Xd, Yd)
    for s in range(3):
        res.gradient_step_range(0, B, STEP, MOMENTUM)
    assert np.array_equal(res.get_weights(), net.get_weights())
    assert np.array_equal(res.get_momentum(), net.get_momentum())

    if dma:
        # The LDS-DMA forms against the register-staged kernels (GNN_MLP_*_DMA=0), masked epilogues included.  bf16: both deal
        # k to the MFMA slots alike and add in the same order -- the same bits.  f32: gemm_f32_dma_kernel adds the same products
        # in another order (test_parity_gpu.py::test_f32_dma_form_against_register_staged_and_oracle) -- its bounds.
        off = _make(gnn, monkeypatch, dt, cls, dims, B, inner, dict(env, GNN_MLP_BF16_DMA="0", GNN_MLP_F32_DMA="0"))
        off.set_weights(w0)
        po = off.propagate(X)
        go = off.calculateWeightGradient(X, Y)
        for s in range(3):
            off.gradientStep(X, STEP, MOMENTUM, False, expected=Y)
        if dt == BF16:
            assert np.array_equal(po, p)
            for l in g:
                assert np.array_equal(go[l], g[l]), "layer %d" % l
            assert np.array_equal(off.get_weights(), net.get_weights())
            assert np.array_equal(off.get_momentum(), net.get_momentum())
        else:
            assert np.abs(po - p).max() <= 1e-5
            for l in g:
                assert np.abs(go[l] - g[l]).max() <= 1e-5 * np.abs(g[l]).max() + 1e-9, "layer %d" % l
            assert np.abs(off.get_weights() - net.get_weights()).max() <= 2e-6
            assert np.abs(off.get_momentum() - net.get_momentum()).max() <= 2e-6


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_large_evaluation_blocks_against_oracle(gnn, dt):
    """Evaluation blocks of 2 048 rows and more (do_forward's big_block): the per-layer GEMM chain + tail_kernel.  784-300-100-10:
    the first layer at M = 2112 on 32x32 tiles (f32) / reg 32x64 (bf16), at M = 4000 on 64x64 tiles; every probability against
    the oracle, and the labels / hit count of the data-set entry where the oracle's top-2 margin is safe."""
    dims = [784, 300, 100, 10]
    tol = TOL[dt]
    fwd, _, _ = _oracle(dt, SCE, LEAKY)
    rng = np.random.default_rng(4242)
    n = 4000
    X = rng.random((n, dims[0])) * (rng.random((n, dims[0])) < 0.3)
    Y = np.eye(dims[-1])[rng.integers(0, dims[-1], n)]
    X32 = X.astype(np.float32).astype(np.float64)
    net = gnn.SoftmaxCrossEntropyNeuralNet(dims, dtype=dt, max_batch=4096)
    net.set_weights(_scaled_weights(net, dims, gain=3.0))
    Ws = np_oracle.split(net.get_weights(), dims)
    net.upload_dataset(X, Y)
    for B in (2100, 4000):
        p = net.propagate(X[:B])
        pref = fwd(Ws, X32[:B])
        assert np.abs(p - pref).max() <= tol["p"], (B, np.abs(p - pref).max())
        srt = np.sort(pref, axis=1)
        safe = (srt[:, -1] - srt[:, -2]) > 2 * tol["p"]      # (softmax is monotone: the logits' order)
        assert safe.mean() > 0.8
        ref_lab = pref.argmax(axis=1)
        lab = net.argmax_range(0, B)
        assert np.array_equal(lab[safe], ref_lab[safe]), B
        hits = net.count_hits_range(0, B)
        truth = Y[:B].argmax(axis=1)
        sure = int((ref_lab == truth)[safe].sum())
        assert sure <= hits <= sure + int((~safe).sum()), (B, hits, sure)
