#!/usr/bin/env python3
"""Measurement tool: integrated gradients on the device (NeuralNet.integrated_gradients_range; csrc/input_grad.hip) against the
host route, the cost of its optional outputs, and against the projected attack with the same number of steps.

The net, rows, warm-up and repeats of tools/bench_pgd.py: 784-300-100-10, f32 and bf16, max_batch 128 and 4096, over --rows
synthetic rows (about 19 % non-zero inputs), baseline 0, steps in --steps (8, 32).  One JSON line per (dtype, max_batch, steps)
with, each a median over --repeats timed calls after --warmup untimed ones and its spread = max - min,
  ig_dev_us      integrated_gradients_range(steps) over all rows: the attributions, one readback
  ig_host_us     the host route: per block of max_batch rows gnn_amd.integrated_gradients (one synchronising gradient call per
                 path point, the sum in numpy)
  ig_delta_us    ... with delta=True (two more forward passes per block and the row sums)
  ig_maps_us     ... with maps=True (the per-class maps and class counts)
  pgd_eval_us    evaluate_pgd_range(eps, eps / 4, steps) over the same rows: the same number of gradient computations
Every (dtype, max_batch) runs in a child process of its own under `timeout`; the tool stops at the first child that fails.
Usage: python tools/bench_integrated_gradients.py [--repeats 5] [--warmup 2] [--rows 10000] [--max-batches 128,4096]
                                                  [--dtypes f32,bf16] [--steps 8,32] [--eps 0.1] [--limit 240]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = [784, 300, 100, 10]


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
    n, mb, eps = a.rows, a.max_batch, a.eps
    d = DIMS[-1]
    dt = {"f32": gnn_amd.DTYPE_F32, "bf16": gnn_amd.DTYPE_BF16}[a.dtype]
    rng = np.random.default_rng(0)
    X = (rng.random((n, DIMS[0])) * (rng.random((n, DIMS[0])) < 0.19)).astype(np.float32).astype(np.float64)
    Y = np.eye(d)[rng.integers(0, d, n)]
    net = gnn_amd.SoftmaxCrossEntropyNeuralNet(DIMS, dtype=dt, max_batch=mb)
    net.upload_dataset(X, Y)
    blocks = [(f, min(mb, n - f)) for f in range(0, n, mb)]

    for m in [int(s) for s in a.steps.split(",")]:
        def ig_dev():
            return net.integrated_gradients_range(m, 0.0, 0, n)

        def ig_delta():
            return net.integrated_gradients_range(m, 0.0, 0, n, delta=True)

        def ig_maps():
            return net.integrated_gradients_range(m, 0.0, 0, n, maps=True)

        def ig_host():
            return np.concatenate([gnn_amd.integrated_gradients(net, X[f:f + b], Y[f:f + b], m) for f, b in blocks])

        def pgd_eval():
            return net.evaluate_pgd_range(eps, eps / 4, m, 0, n)

        same = bool(np.array_equal(ig_dev(), ig_host()))      # (both routes carry the formula in f32 on the same rows)
        gap = float(np.abs(ig_delta()[1]).max())
        dv, dvs = timed(ig_dev, a.warmup, a.repeats)
        dd, dds = timed(ig_delta, a.warmup, a.repeats)
        dm, dms = timed(ig_maps, a.warmup, a.repeats)
        hv, hvs = timed(ig_host, a.warmup, a.repeats)
        pg, pgs = timed(pgd_eval, a.warmup, a.repeats)
        print(json.dumps({
            "shape": "-".join(map(str, DIMS)), "dtype": a.dtype, "n": n, "max_batch": mb, "blocks": len(blocks), "steps": m,
            "step_launches": net.step_launches, "host_route_same_bits": same, "worst_abs_delta": gap,
            "ig_dev_us": round(dv, 1), "ig_dev_spread_us": round(dvs, 1), "ig_host_us": round(hv, 1), "ig_host_spread_us": round(hvs, 1),
            "ig_host_over_dev": round(hv / dv, 2), "ig_delta_us": round(dd, 1), "ig_delta_spread_us": round(dds, 1),
            "ig_delta_over_dev": round(dd / dv, 2), "ig_maps_us": round(dm, 1), "ig_maps_spread_us": round(dms, 1),
            "ig_maps_over_dev": round(dm / dv, 2), "pgd_eval_us": round(pg, 1), "pgd_eval_spread_us": round(pgs, 1),
            "ig_dev_over_pgd": round(dv / pg, 2), "ig_us_per_step_and_block": round(dv / (m * len(blocks)), 2)}), flush=True)
    net.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--max-batches", default="128,4096")
    ap.add_argument("--dtypes", default="f32,bf16")
    ap.add_argument("--steps", default="8,32")
    ap.add_argument("--eps", type=float, default=0.1)
    ap.add_argument("--limit", type=int, default=240, help="seconds a child may run")
    ap.add_argument("--one", action="store_true", help="(internal) measure one dtype / max_batch in this process")
    ap.add_argument("--dtype")
    ap.add_argument("--max-batch", type=int)
    a = ap.parse_args()
    if a.one:
        one(a)
        return 0
    for dn in a.dtypes.split(","):
        for mb in [int(m) for m in a.max_batches.split(",")]:
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--one", "--dtype", dn,
                   "--max-batch", str(mb), "--rows", str(a.rows), "--repeats", str(a.repeats), "--warmup", str(a.warmup),
                   "--steps", a.steps, "--eps", str(a.eps)]
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                print("bench_integrated_gradients: %s max_batch=%d ended with status %d -- stopping" % (dn, mb, rc), file=sys.stderr)
                return rc if rc > 0 else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
