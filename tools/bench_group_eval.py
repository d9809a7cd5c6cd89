#!/usr/bin/env python3
"""Measurement tool: a net group evaluated in one pass (NetGroup.evaluate_range, gnn_mlp_group_evaluate_range) against the way
the same numbers were had before it: K lone count_hits_range calls on the group's members, in the same process and run.

For 784-300-100-10 and 784-100-50-10, f32 and bf16, K in {1, 4, 16}, n in {601, 10 000, 60 000} synthetic rows: one JSON line
per case with
  group_us / lone_us        median over --repeats timed calls after --warmup untimed ones (a call ends with its readback)
  group_spread_us / lone_spread_us   max - min over the repeats
  group_rows_per_s / lone_rows_per_s K * n rows per call, aggregate
  speedup                   lone_us / group_us
  eval_launches             2: the grouped forward kernel applies to the net; 0: member after member
Every (shape, dtype, K) runs in a child process of its own under `timeout`; the tool stops at the first child that fails.
Usage: python tools/bench_group_eval.py [--repeats 5] [--warmup 2] [--ks 1,4,16] [--ns 601,10000,60000] [--shapes A,B]
                                        [--dtypes f32,bf16] [--limit 120]"""
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
    dims, K = SHAPES[a.shape], a.k
    dt = {"f32": gnn_amd.DTYPE_F32, "bf16": gnn_amd.DTYPE_BF16}[a.dtype]
    ns = [int(n) for n in a.ns.split(",")]
    N = max(ns)
    rng = np.random.default_rng(0)
    X = rng.standard_normal((N, dims[0]), dtype=np.float32).astype(np.float64)
    Y = np.eye(dims[-1])[rng.integers(0, dims[-1], N)]
    g = gnn_amd.NetGroup(dims, list(range(1, K + 1)), dtype=dt)
    g.upload_dataset(X, Y)
    for n in ns:
        hits = [None]

        def group_call():
            hits[0] = g.evaluate_range(0, n)[0]

        def lone_call():
            return [m.count_hits_range(0, n) for m in g.members]

        gu, gs = timed(group_call, a.warmup, a.repeats)
        lu, ls = timed(lone_call, a.warmup, a.repeats)
        print(json.dumps({
            "shape": "-".join(map(str, dims)), "dtype": a.dtype, "K": K, "n": n, "eval_launches": g.eval_launches,
            "group_us": round(gu, 1), "group_spread_us": round(gs, 1), "lone_us": round(lu, 1), "lone_spread_us": round(ls, 1),
            "group_rows_per_s": round(K * n / gu * 1e6), "lone_rows_per_s": round(K * n / lu * 1e6),
            "speedup": round(lu / gu, 3),
            "hits_differ_by": int(max(abs(int(h) - l) for h, l in zip(hits[0], lone_call())))}), flush=True)
    g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ks", default="1,4,16")
    ap.add_argument("--ns", default="601,10000,60000")
    ap.add_argument("--shapes", default="A,B")
    ap.add_argument("--dtypes", default="f32,bf16")
    ap.add_argument("--limit", type=int, default=120, help="seconds a child may run")
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
                       "--dtype", dn, "--k", str(K), "--ns", a.ns, "--repeats", str(a.repeats), "--warmup", str(a.warmup)]
                rc = subprocess.run(cmd).returncode
                if rc != 0:
                    print("bench_group_eval: %s %s K=%d ended with status %d -- stopping" % (sh, dn, K, rc), file=sys.stderr)
                    return rc if rc > 0 else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
