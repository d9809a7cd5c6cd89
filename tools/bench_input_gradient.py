#!/usr/bin/env python3
"""Measurement tool: input gradients in one pass (NeuralNet.input_gradient_range, csrc/input_grad_kernel.h) against the
nearest thing the library had before -- the same number of compute_gradient_range calls, which stop at delta_1.

For 784-300-100-10 and 784-100-50-10, f32 and bf16, max_batch 128 and 4096, over --rows synthetic rows (MNIST-like: about 19 %
non-zero inputs): one JSON line per case with, each a median over --repeats timed calls after --warmup untimed ones (a call
ends with its readback or, for (c), with synchronize) and its spread = max - min,
  a_us / a_spread_us   input_gradient_range(grad=False, saliency=True): the maps and the row counts, (d_out + 1) x d_0 numbers back
  b_us / b_spread_us   input_gradient_range(): every row's gradient back (rows x d_0 doubles)
  c_us / c_spread_us   compute_gradient_range per block of max_batch rows, nothing read back: what (a) and (b) run per block
                       before their own launches
  a_minus_c_us, b_minus_c_us, and a_minus_c_per_block_us: what a block's input_grad_kernel + saliency_kernel launches add
Every (shape, dtype, max_batch) runs in a child process of its own under `timeout`; the tool stops at the first child that fails.
The kernels' own times: `rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/bench_input_gradient.py --one ...`,
then tools/rocpd_stats.py DIR/NAME_results.db.
Usage: python tools/bench_input_gradient.py [--repeats 5] [--warmup 2] [--rows 10000] [--max-batches 128,4096]
                                            [--shapes A,B] [--dtypes f32,bf16] [--limit 180]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"A": [784, 300, 100, 10], "B": [784, 100, 50, 10]}


def timed(call, warmup, repeats):
    for _ in range(warmup):
        call()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        t.append((time.perf_counter() - t0) * 1e6)
    t.sort()
    return t[len(t) // 2], t[-1] - t[0]


def one(a):
    import numpy as np
    sys.path.insert(0, ROOT)
    import gnn_amd
    dims, n, mb = SHAPES[a.shape], a.rows, a.max_batch
    d = dims[-1]
    dt = {"f32": gnn_amd.DTYPE_F32, "bf16": gnn_amd.DTYPE_BF16}[a.dtype]
    rng = np.random.default_rng(0)
    X = rng.random((n, dims[0])) * (rng.random((n, dims[0])) < 0.19)
    Y = np.eye(d)[rng.integers(0, d, n)]
    net = gnn_amd.SoftmaxCrossEntropyNeuralNet(dims, dtype=dt, max_batch=mb)
    net.upload_dataset(X, Y)
    del X, Y
    blocks = [(f, min(mb, n - f)) for f in range(0, n, mb)]

    def call_a():
        net.input_gradient_range(0, n, grad=False, saliency=True)

    def call_b():
        net.input_gradient_range(0, n)

    def call_c():
        for f, b in blocks:
            net.compute_gradient_range(f, b)
        net.synchronize()

    au, asp = timed(call_a, a.warmup, a.repeats)
    bu, bsp = timed(call_b, a.warmup, a.repeats)
    cu, csp = timed(call_c, a.warmup, a.repeats)
    print(json.dumps({
        "shape": "-".join(map(str, dims)), "dtype": a.dtype, "n": n, "max_batch": mb, "blocks": len(blocks),
        "step_launches": net.step_launches,
        "a_us": round(au, 1), "a_spread_us": round(asp, 1), "b_us": round(bu, 1), "b_spread_us": round(bsp, 1),
        "c_us": round(cu, 1), "c_spread_us": round(csp, 1), "a_minus_c_us": round(au - cu, 1), "b_minus_c_us": round(bu - cu, 1),
        "a_minus_c_per_block_us": round((au - cu) / len(blocks), 2)}), flush=True)
    net.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--max-batches", default="128,4096")
    ap.add_argument("--shapes", default="A,B")
    ap.add_argument("--dtypes", default="f32,bf16")
    ap.add_argument("--limit", type=int, default=180, help="seconds a child may run")
    ap.add_argument("--one", action="store_true", help="(internal) measure one shape / dtype / max_batch in this process")
    ap.add_argument("--shape")
    ap.add_argument("--dtype")
    ap.add_argument("--max-batch", type=int)
    a = ap.parse_args()
    if a.one:
        one(a)
        return 0
    for sh in a.shapes.split(","):
        for dn in a.dtypes.split(","):
            for mb in [int(m) for m in a.max_batches.split(",")]:
                cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--one", "--shape", sh,
                       "--dtype", dn, "--max-batch", str(mb), "--rows", str(a.rows),
                       "--repeats", str(a.repeats), "--warmup", str(a.warmup)]
                rc = subprocess.run(cmd).returncode
                if rc != 0:
                    print("bench_input_gradient: %s %s max_batch=%d ended with status %d -- stopping" % (sh, dn, mb, rc), file=sys.stderr)
                    return rc if rc > 0 else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
