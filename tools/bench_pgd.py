#!/usr/bin/env python3
"""Measurement tool: the projected-gradient calls on the device (NeuralNet.evaluate_pgd_range, train_sampled_pgd;
csrc/adversarial.hip) against the host route and against the one-step (FGSM) calls.

The net, rows, eps, warm-up and repeats of tools/bench_adversarial.py: 784-300-100-10, f32 and bf16, max_batch 128 and 4096, over
--rows synthetic rows (about 19 % non-zero inputs).  alpha = eps / 4, steps in --steps (1, 4, 10).  One JSON line per
(dtype, max_batch, steps) with, each a median over --repeats timed calls after --warmup untimed ones and its spread = max - min,
  eval_dev_us     evaluate_pgd_range(eps, alpha, steps) over all rows: robust hits and loss, one readback of two numbers
  eval_host_us    the host route: per block of max_batch rows gnn_amd.pgd (one synchronising gradient call per step, the step in
                  numpy), then calculateLoss and argmax on the attacked rows as host batches
  eval_fgsm_us    evaluate_fgsm_range(eps) over the same rows
  eval_curve_us   evaluate_pgd_range(..., curve=True): steps + 1 entries
  train_pgd_us_per_iteration / train_fgsm_us_per_iteration / train_us_per_iteration   train_sampled_pgd / train_sampled_fgsm /
                  train_sampled, --iterations iterations of batch --batch per timed call, divided by the iterations
Every (dtype, max_batch) runs in a child process of its own under `timeout`; the tool stops at the first child that fails.
Usage: python tools/bench_pgd.py [--repeats 5] [--warmup 2] [--rows 10000] [--max-batches 128,4096] [--dtypes f32,bf16]
                                 [--steps 1,4,10] [--iterations 300] [--batch 128] [--eps 0.1] [--limit 240]"""
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
    alpha = eps / 4
    d = DIMS[-1]
    dt = {"f32": gnn_amd.DTYPE_F32, "bf16": gnn_amd.DTYPE_BF16}[a.dtype]
    rng = np.random.default_rng(0)
    X = rng.random((n, DIMS[0])) * (rng.random((n, DIMS[0])) < 0.19)
    Y = np.eye(d)[rng.integers(0, d, n)]
    net = gnn_amd.SoftmaxCrossEntropyNeuralNet(DIMS, dtype=dt, max_batch=mb)
    net.upload_dataset(X, Y)
    expected = Y.argmax(axis=1)
    blocks = [(f, min(mb, n - f)) for f in range(0, n, mb)]
    smp = gnn_amd.Sampler(n, seed=1)
    batch = min(a.batch, mb)
    it = float(a.iterations)

    def eval_fgsm():
        return net.evaluate_fgsm_range(eps, 0, n)

    def train_fgsm():
        net.train_sampled_fgsm(smp, a.iterations, batch, 0.0125, 0.9, eps)
        net.synchronize()

    def train_plain():
        net.train_sampled(smp, a.iterations, batch, 0.0125, 0.9)
        net.synchronize()

    for T in [int(s) for s in a.steps.split(",")]:
        def eval_dev():
            return net.evaluate_pgd_range(eps, alpha, T, 0, n)

        def eval_curve():
            return net.evaluate_pgd_range(eps, alpha, T, 0, n, curve=True)

        def eval_host():
            hits, loss = 0, 0.0
            for f, b in blocks:
                adv = gnn_amd.pgd(net, X[f:f + b], Y[f:f + b], eps, alpha, T, first_row=f)
                loss += float(np.sum(net.calculateLoss(adv, Y[f:f + b])))
                hits += int((net.argmax(adv) == expected[f:f + b]).sum())
            return hits, loss

        def train_pgd():
            net.train_sampled_pgd(smp, a.iterations, batch, 0.0125, 0.9, eps, alpha, T)
            net.synchronize()

        dev, host = eval_dev(), eval_host()     # (both routes carry the step in f32 on rows the device holds in f32: the same hits)
        ed, eds = timed(eval_dev, a.warmup, a.repeats)
        ec, ecs = timed(eval_curve, a.warmup, a.repeats)
        eh, ehs = timed(eval_host, a.warmup, a.repeats)
        ef, efs = timed(eval_fgsm, a.warmup, a.repeats)
        tg, tgs = timed(train_pgd, a.warmup, a.repeats)
        tf, tfs = timed(train_fgsm, a.warmup, a.repeats)
        tp, tps = timed(train_plain, a.warmup, a.repeats)
        print(json.dumps({
            "shape": "-".join(map(str, DIMS)), "dtype": a.dtype, "n": n, "max_batch": mb, "blocks": len(blocks), "steps": T,
            "step_launches": net.step_launches, "hits_dev": dev[0], "hits_host": host[0],
            "eval_dev_us": round(ed, 1), "eval_dev_spread_us": round(eds, 1), "eval_host_us": round(eh, 1), "eval_host_spread_us": round(ehs, 1),
            "eval_host_over_dev": round(eh / ed, 2), "eval_fgsm_us": round(ef, 1), "eval_fgsm_spread_us": round(efs, 1),
            "eval_dev_over_fgsm": round(ed / ef, 2), "eval_curve_us": round(ec, 1), "eval_curve_spread_us": round(ecs, 1),
            "eval_curve_over_dev": round(ec / ed, 2), "iterations": a.iterations, "batch": batch,
            "train_pgd_us_per_iteration": round(tg / it, 2), "train_pgd_spread_us": round(tgs / it, 2),
            "train_fgsm_us_per_iteration": round(tf / it, 2), "train_fgsm_spread_us": round(tfs / it, 2),
            "train_us_per_iteration": round(tp / it, 2), "train_spread_us": round(tps / it, 2),
            "train_pgd_over_fgsm": round(tg / tf, 2), "train_pgd_over_train": round(tg / tp, 2)}), flush=True)
    net.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--max-batches", default="128,4096")
    ap.add_argument("--dtypes", default="f32,bf16")
    ap.add_argument("--steps", default="1,4,10")
    ap.add_argument("--iterations", type=int, default=300)
    ap.add_argument("--batch", type=int, default=128)
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
                   "--steps", a.steps, "--iterations", str(a.iterations), "--batch", str(a.batch), "--eps", str(a.eps)]
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                print("bench_pgd: %s max_batch=%d ended with status %d -- stopping" % (dn, mb, rc), file=sys.stderr)
                return rc if rc > 0 else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
