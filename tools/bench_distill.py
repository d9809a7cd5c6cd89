#!/usr/bin/env python3
"""Measurement tool: an ensemble's outputs written into a student's resident targets (NeuralNet.distill_from,
csrc/distill.hip) against the only route there was before it.

784-300-100-10 teachers, K in {1, 4, 16} (a NetGroup), distilled with keep = 0.1 into a 784-100-50-10 student over --rows
synthetic rows, f32 and bf16: one JSON line per case with, each a median over --repeats timed calls after --warmup untimed ones
and its spread = max - min,
  a_us / a_spread_us   route A: student.distill_from(group, keep) -- gnn_mlp_group_distill_range: the teachers' evaluation pass
                       on the student's resident inputs and the blend, all on the device; synchronous
  b_us / b_spread_us   route B: group.ensemble_propagate_range to the host, the blend in numpy, student.upload_dataset with the
                       fp64 inputs again (the group holds its own copy of the rows for this route)
  b_over_a, and targets_max_diff: the largest difference between the targets the two routes leave (fp64 blend against f32)
Every (dtype, K) runs in a child process of its own under `timeout`; the tool stops at the first child that fails.
Usage: python tools/bench_distill.py [--repeats 5] [--warmup 2] [--ks 1,4,16] [--rows 60000] [--max-batch 128]
                                     [--dtypes f32,bf16] [--keep 0.1] [--limit 240]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEACHER, STUDENT = [784, 300, 100, 10], [784, 100, 50, 10]


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
    K, n, mb, keep = a.k, a.rows, a.max_batch, a.keep
    d = STUDENT[-1]
    dt = {"f32": gnn_amd.DTYPE_F32, "bf16": gnn_amd.DTYPE_BF16}[a.dtype]
    rng = np.random.default_rng(0)
    X = rng.standard_normal((n, STUDENT[0]), dtype=np.float32).astype(np.float64)
    Y = np.eye(d)[rng.integers(0, d, n)]
    g = gnn_amd.NetGroup(TEACHER, list(range(1, K + 1)), dtype=dt, max_batch=mb)
    g.upload_dataset(X, Y)                      # (route B reads the group's own copy)
    s = gnn_amd.SoftmaxCrossEntropyNeuralNet(STUDENT, dtype=dt, max_batch=mb)
    s.upload_dataset(X, Y)
    got = [None, None]

    def call_a():                               # (the time does not depend on the values: no reset between the calls)
        s.distill_from(g, keep=keep)

    def call_b():
        mean = g.ensemble_propagate_range(0, n)
        s.upload_dataset(X, keep * Y + (1.0 - keep) * mean)

    au, asp = timed(call_a, a.warmup, a.repeats)
    s.set_targets(Y)                            # one call from the one-hot rows, for the comparison of what the routes leave
    s.distill_from(g, keep=keep)
    got[0] = s.get_targets()
    bu, bsp = timed(call_b, a.warmup, a.repeats)
    got[1] = s.get_targets()
    print(json.dumps({
        "teacher": "-".join(map(str, TEACHER)), "student": "-".join(map(str, STUDENT)), "dtype": a.dtype, "K": K, "n": n,
        "max_batch": mb, "keep": keep, "eval_launches": g.eval_launches,
        "a_us": round(au, 1), "a_spread_us": round(asp, 1),
        "b_us": round(bu, 1), "b_spread_us": round(bsp, 1), "b_over_a": round(bu / au, 2),
        "targets_max_diff": float(np.abs(got[0] - got[1]).max())}), flush=True)
    s.close()
    g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ks", default="1,4,16")
    ap.add_argument("--rows", type=int, default=60000)
    ap.add_argument("--max-batch", type=int, default=128)
    ap.add_argument("--dtypes", default="f32,bf16")
    ap.add_argument("--keep", type=float, default=0.1)
    ap.add_argument("--limit", type=int, default=240, help="seconds a child may run")
    ap.add_argument("--one", action="store_true", help="(internal) measure one dtype / K in this process")
    ap.add_argument("--dtype")
    ap.add_argument("--k", type=int)
    a = ap.parse_args()
    if a.one:
        one(a)
        return 0
    for dn in a.dtypes.split(","):
        for K in [int(k) for k in a.ks.split(",")]:
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--one", "--dtype", dn,
                   "--k", str(K), "--rows", str(a.rows), "--max-batch", str(a.max_batch), "--keep", str(a.keep),
                   "--repeats", str(a.repeats), "--warmup", str(a.warmup)]
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                print("bench_distill: %s K=%d ended with status %d -- stopping" % (dn, K, rc), file=sys.stderr)
                return rc if rc > 0 else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
