#!/usr/bin/env python3
"""Measurement tool: K nets of one shape trained side by side (NetGroup, gnn_mlp_group_*) against the same K nets stepped
one after another in the same process.

For 784-300-100-10 and 784-100-50-10, f32 and bf16, B = 128, K in {1, 2, 4, 8, 16}: one JSON line per case with
  group_us_per_step   one group step: a synchronised run of --steps steps after --warmup, divided by --steps (the loop is
                      bound by the device: the host enqueues a step in a fraction of its time)
  lone_us_per_step    the same K nets as lone handles, one synchronised run after the other: the sum of their times per step
  group_us_per_step_events   cross-check of the first: device events recorded on the group's stream around every group step
                      (gnn_mlp_timing_enable on member 0, class GNN_K_STEP), mean over --steps steps.  (No such figure for
                      the lone handles: with timing on, a lone handle also times every kernel of its step, which slows it.)
  group_samples_per_s / lone_samples_per_s   K * B samples per step, aggregate
  speedup             lone_us_per_step / group_us_per_step
Usage: python tools/bench_group.py [--steps 2000] [--warmup 200] [--ks 1,2,4,8,16] [--shapes A,B] [--dtypes f32,bf16]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gnn_amd  # noqa: E402

SHAPES = {"A": [784, 300, 100, 10], "B": [784, 100, 50, 10]}
DTYPES = {"f32": gnn_amd.DTYPE_F32, "bf16": gnn_amd.DTYPE_BF16}
GNN_K_STEP = 2


def events_us(net, run):
    """mean device time per step of `run` (events around every step on the net's stream)"""
    net.timing_enable(True)
    run()
    mean, count = net.timing_read(GNN_K_STEP)
    net.timing_enable(False)
    return mean, count


def wall_us(sync, run, steps):
    sync()
    t0 = time.perf_counter()
    run()
    sync()
    return (time.perf_counter() - t0) / steps * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--ks", default="1,2,4,8,16")
    ap.add_argument("--shapes", default="A,B")
    ap.add_argument("--dtypes", default="f32,bf16")
    a = ap.parse_args()
    B, S, W = a.batch, a.steps, a.warmup
    N = B * 50
    rng = np.random.default_rng(0)
    X = rng.random((N, 784))
    Y = np.eye(10)[rng.integers(0, 10, N)]
    for sh in a.shapes.split(","):
        dims = SHAPES[sh]
        for dn in a.dtypes.split(","):
            dt = DTYPES[dn]
            for K in [int(k) for k in a.ks.split(",")]:
                steps = [0.0125 * (1 + 0.1 * k) for k in range(K)]
                moms = [0.9] * K
                g = gnn_amd.NetGroup(dims, list(range(1, K + 1)), dtype=dt, max_batch=B)
                g.upload_dataset(X, Y)
                g.train_range(0, B, W, steps, moms)
                gw = wall_us(g.synchronize, lambda: g.train_range(0, B, S, steps, moms), S)
                ge, gcount = events_us(g.members[0], lambda: (g.train_range(0, B, S, steps, moms), g.synchronize()))
                lpg = g.launches_per_step
                g.close()
                lone = 0.0
                for k in range(K):
                    n = gnn_amd.SoftmaxCrossEntropyNeuralNet(dims, seed=k + 1, dtype=dt, max_batch=B)
                    n.upload_dataset(X, Y)
                    n.train_range(0, B, W, steps[k], moms[k])
                    lone += wall_us(n.synchronize, lambda: n.train_range(0, B, S, steps[k], moms[k]), S)
                    n.close()
                print(json.dumps({
                    "shape": "-".join(map(str, dims)), "dtype": dn, "B": B, "K": K, "steps": S, "launches_per_step": lpg,
                    "group_us_per_step": round(gw, 2), "lone_us_per_step": round(lone, 2),
                    "group_us_per_step_events": round(ge, 2), "group_steps_timed": gcount,
                    "group_samples_per_s": round(K * B / gw * 1e6), "lone_samples_per_s": round(K * B / lone * 1e6),
                    "speedup": round(lone / gw, 3)}), flush=True)


if __name__ == "__main__":
    main()
