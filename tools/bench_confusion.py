#!/usr/bin/env python3
"""Measurement tool: confusion matrices in one pass (NeuralNet.confusion_range / NetGroup.confusion_range,
csrc/confusion_kernel.h) against the same evaluation pass without them and against the way the same matrices were had before.

For 784-300-100-10 and 784-100-50-10, f32 and bf16, K in {1, 8, 16} over --rows synthetic rows (K = 1 is a lone handle, K > 1
a NetGroup; every handle with --max-batch rows): one JSON line per case with, each a median over --repeats timed calls after
--warmup untimed ones (a call ends with its readback) and its spread = max - min,
  a_us / a_spread_us   confusion_range: every member's matrix and the ensemble's
  b_us / b_spread_us   the same pass without the confusion launch: NetGroup.evaluate_range (K = 1: count_hits_range on the
                       lone handle, which computes no loss either)
  c_us / c_spread_us   the matrices without this kernel: argmax_range in blocks of max_batch per member -- a wait and a
                       readback per block -- and a numpy histogram per member (no ensemble matrix)
  a_minus_b_us, c_over_a, and rows_counted_differently: rows that (a) and (c) put into different cells (the two take different
                       forward kernels, which agree up to f32 summation order: near-ties only)
Every (shape, dtype, K) runs in a child process of its own under `timeout`; the tool stops at the first child that fails.
Usage: python tools/bench_confusion.py [--repeats 5] [--warmup 2] [--ks 1,8,16] [--rows 60000] [--max-batch 128]
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
    dims, K, n, mb = SHAPES[a.shape], a.k, a.rows, a.max_batch
    d = dims[-1]
    dt = {"f32": gnn_amd.DTYPE_F32, "bf16": gnn_amd.DTYPE_BF16}[a.dtype]
    rng = np.random.default_rng(0)
    X = rng.standard_normal((n, dims[0]), dtype=np.float32).astype(np.float64)
    cls = rng.integers(0, d, n)
    Y = np.eye(d)[cls]
    if K == 1:
        g = None
        nets = [gnn_amd.SoftmaxCrossEntropyNeuralNet(dims, dtype=dt, max_batch=mb)]
        nets[0].upload_dataset(X, Y)
    else:
        g = gnn_amd.NetGroup(dims, list(range(1, K + 1)), dtype=dt, max_batch=mb)
        g.upload_dataset(X, Y)
        nets = g.members
    del X, Y
    got = [None, None]

    def call_a():
        got[0] = nets[0].confusion_range(0, n)[None] if g is None else g.confusion_range(0, n)[0]

    def call_b():
        return nets[0].count_hits_range(0, n) if g is None else g.evaluate_range(0, n)

    def call_c():
        out = np.zeros((K, d, d), dtype=np.int64)
        for k, m in enumerate(nets):
            lab = np.concatenate([m.argmax_range(f, min(mb, n - f)) for f in range(0, n, mb)])
            np.add.at(out[k], (cls, lab), 1)
        got[1] = out

    au, asp = timed(call_a, a.warmup, a.repeats)
    bu, bsp = timed(call_b, a.warmup, a.repeats)
    cu, csp = timed(call_c, a.warmup, a.repeats)
    print(json.dumps({
        "shape": "-".join(map(str, dims)), "dtype": a.dtype, "K": K, "n": n, "max_batch": mb,
        "eval_launches": -1 if g is None else g.eval_launches,
        "a_us": round(au, 1), "a_spread_us": round(asp, 1), "b_us": round(bu, 1), "b_spread_us": round(bsp, 1),
        "c_us": round(cu, 1), "c_spread_us": round(csp, 1), "a_minus_b_us": round(au - bu, 1), "c_over_a": round(cu / au, 2),
        "a_below_c_by_more_than_both_spreads": bool(cu - au > asp and cu - au > csp),
        "rows_counted_differently": int(np.abs(got[0] - got[1]).sum() // 2)}), flush=True)
    if g is None:
        nets[0].close()
    else:
        g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ks", default="1,8,16")
    ap.add_argument("--rows", type=int, default=60000)
    ap.add_argument("--max-batch", type=int, default=128)
    ap.add_argument("--shapes", default="A,B")
    ap.add_argument("--dtypes", default="f32,bf16")
    ap.add_argument("--limit", type=int, default=180, help="seconds a child may run")
    ap.add_argument("--one", action="store_true", help="(internal) measure one shape / dtype / K in this process")
    ap.add_argument("--shape")
    ap.add_argument("--dtype")
    ap.add_argument("--k", type=int)
    a = ap.parse_args()
    if a.one:
        one(a)
        return 0
    for sh in a.shapes.split(","):
        for dn in a.dtypes.split(","):
            for K in [int(k) for k in a.ks.split(",")]:
                cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--one", "--shape", sh,
                       "--dtype", dn, "--k", str(K), "--rows", str(a.rows), "--max-batch", str(a.max_batch),
                       "--repeats", str(a.repeats), "--warmup", str(a.warmup)]
                rc = subprocess.run(cmd).returncode
                if rc != 0:
                    print("bench_confusion: %s %s K=%d ended with status %d -- stopping" % (sh, dn, K, rc), file=sys.stderr)
                    return rc if rc > 0 else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
