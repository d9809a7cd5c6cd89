#!/usr/bin/env python3
"""Measurement tool: the observed training loop (NNT:68-79: sample, gradientStep, validate per iteration) of a net group in
grouped launches (NetGroup.train_sampled_observed, gnn_mlp_group_train_sampled_observed) against what there was before it.

For 784-300-100-10 and 784-100-50-10, f32 and bf16, K in {1, 4, 8, 16}; batch 128 over 60 000 synthetic rows, validation on
601 rows (MNIST's sizes), --iterations per timed call after one untimed call of --warm iterations: one JSON line per case with
  group_us / lone_us / plain_us   per ITERATION, median over --repeats timed calls (a call ends with its readback):
                                  (a) the group call; (b) K gnn_mlp_train_sampled_observed loops one after the other on the
                                  group's members, each with its own sampler; (c) NetGroup.train_sampled, no validation
  *_spread_us                     max - min over the repeats
  speedup                         lone_us / group_us
  group_beats_lone                the group's median lies below the K lone loops' by more than the larger of the two spreads
  observed_launches               3: grouped step and validation launches; 0: member after member
Every (shape, dtype, K) runs in a child process of its own under `timeout`; the tool stops at the first child that fails.
`--one --forms a --repeats 1 --warm 0` is one group call alone in this process (for a kernel trace).
Usage: python tools/bench_group_observed.py [--iterations 2000] [--warm 200] [--repeats 5] [--ks 1,4,8,16] [--shapes A,B]
                                            [--dtypes f32,bf16] [--limit 300]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"A": [784, 300, 100, 10], "B": [784, 100, 50, 10]}
N, BATCH, V = 60000, 128, 601


def timed(call, repeats, iterations):
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call(iterations)
        t.append((time.perf_counter() - t0) * 1e6 / iterations)
    t.sort()
    return t[len(t) // 2], t[-1] - t[0]


def one(a):
    import numpy as np
    sys.path.insert(0, ROOT)
    import gnn_amd
    dims, K = SHAPES[a.shape], a.k
    dt = {"f32": gnn_amd.DTYPE_F32, "bf16": gnn_amd.DTYPE_BF16}[a.dtype]
    rng = np.random.default_rng(0)
    pix = rng.integers(0, 256, (N, dims[0]), dtype=np.uint8)
    pix[rng.random((N, dims[0])) < 0.8] = 0
    lab = rng.integers(0, dims[-1], N, dtype=np.uint8)
    steps = [0.005 * (1 + k / K) for k in range(K)]
    moms = [0.9 - 0.02 * k for k in range(K)]
    g = gnn_amd.NetGroup(dims, list(range(1, K + 1)), dtype=dt, max_batch=BATCH)
    g.upload_dataset_u8(pix, lab)
    s = gnn_amd.Sampler(N, seed=1)
    lone_s = [gnn_amd.Sampler(N, seed=1) for _ in range(K)]
    lib = gnn_amd.load_library()

    def group_call(n):
        return g.train_sampled_observed(s, n, BATCH, steps, moms, V)

    def lone_call(n):
        val = np.empty(n)
        for k, m in enumerate(g.members):
            gnn_amd._capi.check(lib.gnn_mlp_train_sampled_observed(m._h, lone_s[k]._h, n, BATCH, steps[k], moms[k], 0, V,
                                                                   val.ctypes.data_as(C.POINTER(C.c_double))))

    def plain_call(n):
        g.train_sampled(s, n, BATCH, steps, moms)
        g.synchronize()

    forms = {"a": ("group", group_call), "b": ("lone", lone_call), "c": ("plain", plain_call)}
    row = {"shape": "-".join(map(str, dims)), "dtype": a.dtype, "K": K, "iterations": a.iterations,
           "observed_launches": g.observed_launches}
    for f in a.forms.split(","):
        name, call = forms[f]
        if a.warm > 0:
            call(a.warm)
        med, spread = timed(call, a.repeats, a.iterations)
        row[name + "_us"], row[name + "_spread_us"] = round(med, 2), round(spread, 2)
    if "group_us" in row and "lone_us" in row:
        row["speedup"] = round(row["lone_us"] / row["group_us"], 3)
        row["group_beats_lone"] = bool(row["lone_us"] - row["group_us"] > max(row["group_spread_us"], row["lone_spread_us"]))
    print(json.dumps(row), flush=True)
    g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=2000)
    ap.add_argument("--warm", type=int, default=200, help="iterations of the untimed call in front of each form's timed ones")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ks", default="1,4,8,16")
    ap.add_argument("--shapes", default="A,B")
    ap.add_argument("--dtypes", default="f32,bf16")
    ap.add_argument("--forms", default="a,b,c")
    ap.add_argument("--limit", type=int, default=300, help="seconds a child may run")
    ap.add_argument("--one", action="store_true", help="measure one shape / dtype / K in this process")
    ap.add_argument("--shape", default="A")
    ap.add_argument("--dtype", default="f32")
    ap.add_argument("--k", type=int, default=8)
    a = ap.parse_args()
    if a.one:
        one(a)
        return 0
    for sh in a.shapes.split(","):
        for dn in a.dtypes.split(","):
            for K in [int(k) for k in a.ks.split(",")]:
                cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--one", "--shape", sh,
                       "--dtype", dn, "--k", str(K), "--iterations", str(a.iterations), "--warm", str(a.warm),
                       "--repeats", str(a.repeats), "--forms", a.forms]
                rc = subprocess.run(cmd).returncode
                if rc != 0:
                    print("bench_group_observed: %s %s K=%d ended with status %d -- stopping" % (sh, dn, K, rc), file=sys.stderr)
                    return rc if rc > 0 else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
