#!/usr/bin/env python3
"""Measurement tool: a training loop with a held-out curve and the best weights kept on the device
(NeuralNet.train_sampled_held_out / NetGroup.train_sampled_held_out, csrc/keep_best_kernel.h) against the nearest thing the
library had before, which could hold one resident set and decided on the host.

For 784-300-100-10 and 784-100-50-10, f32 and bf16, 60 000 training + 10 000 held-out synthetic rows (MNIST-like: about 19 %
non-zero inputs), batch 128, --iterations iterations, a lone net and a group of --members nets, `every` in --every: one JSON line
per case with, each a median over --repeats timed calls after --warmup untimed ones and its spread = max - min,
  a_us / a_spread_us   the new call: the curve over all held-out rows, the best point, the best weights back
  b_us / b_spread_us   per point: train_sampled(every) + evaluate_range(0, 10 000) on the TRAINING set (the one resident set
                       the library had) + get_weights (of every member) -- a synchronisation, two readbacks and a restart of
                       the step chain behind every point
  c_us / c_spread_us   train_sampled alone (measured once per net: it does not depend on `every`)
  b_minus_a_per_point_us   what the device-side selection saves per point
  a_minus_c_per_point_us   what a point costs: about one evaluation pass of 10 000 rows plus one copy of the weights
Every (shape, dtype, lone / group) runs in a child process of its own under `timeout`; the tool stops at the first child that
fails.  The kernels' own times: `rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/bench_held_out.py --one ...`
(a run of its own, never combined with counters), then tools/rocpd_stats.py DIR/NAME_results.db.
Usage: python tools/bench_held_out.py [--repeats 5] [--warmup 2] [--iterations 2000] [--every 10,100,1000] [--members 8]
                                      [--shapes A,B] [--dtypes f32,bf16] [--who lone,group] [--limit 420]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"A": [784, 300, 100, 10], "B": [784, 100, 50, 10]}
TRAIN_ROWS, HELD_ROWS, BATCH, STEP, MOMENTUM = 60000, 10000, 128, 0.0125, 0.9


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
    dims, it = SHAPES[a.shape], a.iterations
    d = dims[-1]
    dt = {"f32": gnn_amd.DTYPE_F32, "bf16": gnn_amd.DTYPE_BF16}[a.dtype]
    K = a.members if a.who == "group" else 1
    rng = np.random.default_rng(0)

    def rows(n):
        return (rng.random((n, dims[0]), dtype=np.float32) * (rng.random((n, dims[0]), dtype=np.float32) < 0.19)).astype(np.float64), \
            np.eye(d)[rng.integers(0, d, n)]

    if a.who == "group":
        net = gnn_amd.NetGroup(dims, list(range(1, K + 1)), dtype=dt, max_batch=BATCH)
        samplers = [gnn_amd.Sampler(TRAIN_ROWS, seed=k + 1) for k in range(K)]
    else:
        net = gnn_amd.SoftmaxCrossEntropyNeuralNet(dims, dtype=dt, max_batch=BATCH)
        samplers = gnn_amd.Sampler(TRAIN_ROWS, seed=1)
    X, Y = rows(TRAIN_ROWS)
    net.upload_dataset(X, Y)
    del X, Y
    X, Y = rows(HELD_ROWS)
    net.upload_held_out(X, Y)
    del X, Y

    def train(n):
        if a.who == "group":
            net.train_sampled(samplers, n, [BATCH] * K, STEP, MOMENTUM)
        else:
            gnn_amd._capi.check(net._lib.gnn_mlp_train_sampled(net._h, samplers._h, n, BATCH, STEP, MOMENTUM, 0))

    def call_c():
        train(it)
        net.synchronize()

    cu, csp = timed(call_c, a.warmup, a.repeats)
    for every in [int(e) for e in a.every.split(",")]:
        points = (it + every - 1) // every

        def call_a():  # (the same signature on a net and on a group)
            net.train_sampled_held_out(samplers, it, BATCH, STEP, MOMENTUM, every)

        def call_b():
            done = 0
            while done < it:
                n = min(every, it - done)
                train(n)
                done += n
                net.evaluate_range(0, HELD_ROWS)
                if a.who == "group":
                    for m in net.members:
                        m.get_weights()
                else:
                    net.get_weights()

        au, asp = timed(call_a, a.warmup, a.repeats)
        bu, bsp = timed(call_b, a.warmup, a.repeats)
        print(json.dumps({
            "shape": "-".join(map(str, dims)), "dtype": a.dtype, "who": a.who, "K": K, "iterations": it, "every": every, "points": points,
            "a_us": round(au, 1), "a_spread_us": round(asp, 1), "b_us": round(bu, 1), "b_spread_us": round(bsp, 1),
            "c_us": round(cu, 1), "c_spread_us": round(csp, 1),
            "b_minus_a_per_point_us": round((bu - au) / points, 2), "a_minus_c_per_point_us": round((au - cu) / points, 2)}), flush=True)
    net.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iterations", type=int, default=2000)
    ap.add_argument("--every", default="10,100,1000")
    ap.add_argument("--members", type=int, default=8)
    ap.add_argument("--shapes", default="A,B")
    ap.add_argument("--dtypes", default="f32,bf16")
    ap.add_argument("--who", default="lone,group")
    ap.add_argument("--limit", type=int, default=420, help="seconds a child may run")
    ap.add_argument("--one", action="store_true", help="(internal) measure one shape / dtype / lone-or-group in this process")
    ap.add_argument("--shape")
    ap.add_argument("--dtype")
    a = ap.parse_args()
    if a.one:
        one(a)
        return 0
    for sh in a.shapes.split(","):
        for dn in a.dtypes.split(","):
            for who in a.who.split(","):
                cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--one", "--shape", sh,
                       "--dtype", dn, "--who", who, "--iterations", str(a.iterations), "--every", a.every, "--members", str(a.members),
                       "--repeats", str(a.repeats), "--warmup", str(a.warmup)]
                rc = subprocess.run(cmd).returncode
                if rc != 0:
                    print("bench_held_out: %s %s %s ended with status %d -- stopping" % (sh, dn, who, rc), file=sys.stderr)
                    return rc if rc > 0 else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
