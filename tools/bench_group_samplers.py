#!/usr/bin/env python3
"""Measurement tool: a NetGroup trained with ONE SAMPLER PER MEMBER (NetGroup.train_sampled([s_0 .. s_{K-1}], ..),
gnn_mlp_group_train_sampled_each) against the same group with one shared sampler and against the K nets as lone runs.

For 784-300-100-10 and 784-100-50-10, f32 and bf16, K in {2, 8, 16}, B in {16, 128} (16: the reference's batch, MT:228) on
60 000 synthetic rows: one JSON line per case with, per iteration of a synchronised run of --iterations after --warmup,
  each_us     (a) the group, member k drawing from its own sampler (seed k + 1)
  shared_us   (b) the same group with ONE sampler for all: the same launches, one sampler -- the ceiling of (a)
  lone_us     (c) the K nets as lone handles, train_sampled one after another with their own samplers: the sum of their times
  grouped / member_after_member   how (a)'s iterations were stepped (NetGroup.sampled_each_iterations)
  sampler_us_per_batch   one sampler drawing batches of B on ONE host thread, through the Python binding (its call overhead of
              about a microsecond included); chunk_ms_per_thread = that for a full chunk of 256 iterations times the
              ceil(K / 8) members a worker thread draws for -- to be compared with 256 * each_us
Usage: python tools/bench_group_samplers.py [--iterations 2000] [--warmup 200] [--ks 2,8,16] [--batches 16,128]
                                            [--shapes A,B] [--dtypes f32,bf16] [--rows 60000]"""
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


def wall_us(sync, run, iterations):
    sync()
    t0 = time.perf_counter()
    run()
    sync()
    return (time.perf_counter() - t0) / iterations * 1e6


def sampler_us(rows, B, batches=2048):
    s = gnn_amd.Sampler(rows, seed=1)
    for _ in range(64):
        s.sample(B)
    t0 = time.perf_counter()
    for _ in range(batches):
        s.sample(B)
    us = (time.perf_counter() - t0) / batches * 1e6
    s.close()
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--ks", default="2,8,16")
    ap.add_argument("--batches", default="16,128")
    ap.add_argument("--shapes", default="A,B")
    ap.add_argument("--dtypes", default="f32,bf16")
    ap.add_argument("--rows", type=int, default=60000)
    a = ap.parse_args()
    S, W, N = a.iterations, a.warmup, a.rows
    rng = np.random.default_rng(0)
    pix = rng.integers(0, 256, (N, 784), dtype=np.uint8)
    lab = rng.integers(0, 10, N, dtype=np.uint8)
    per_batch = {B: sampler_us(N, B) for B in [int(b) for b in a.batches.split(",")]}
    for sh in a.shapes.split(","):
        dims = SHAPES[sh]
        for dn in a.dtypes.split(","):
            dt = DTYPES[dn]
            for B in [int(b) for b in a.batches.split(",")]:
                for K in [int(k) for k in a.ks.split(",")]:
                    steps = [0.0125 * (1 + 0.1 * k) for k in range(K)]
                    moms = [0.9] * K
                    g = gnn_amd.NetGroup(dims, list(range(1, K + 1)), dtype=dt, max_batch=B)
                    g.upload_dataset_u8(pix, lab)
                    own = [gnn_amd.Sampler(N, seed=k + 1) for k in range(K)]
                    one = gnn_amd.Sampler(N, seed=1)
                    g.train_sampled(own, W, B, steps, moms)
                    each = wall_us(g.synchronize, lambda: g.train_sampled(own, S, B, steps, moms), S)
                    grouped, mixed = g.sampled_each_iterations
                    g.train_sampled(one, W, B, steps, moms)
                    shared = wall_us(g.synchronize, lambda: g.train_sampled(one, S, B, steps, moms), S)
                    lpg = g.launches_per_step
                    for x in own + [one, g]:
                        x.close()
                    lone = 0.0
                    for k in range(K):
                        n = gnn_amd.SoftmaxCrossEntropyNeuralNet(dims, seed=k + 1, dtype=dt, max_batch=B)
                        tr = gnn_amd.NeuralNetTrainer(pix, lab, n, raw_u8=True, seed=k + 1)
                        tr.train(W, steps[k], B, moms[k])
                        lone += wall_us(n.synchronize, lambda: tr.train(S, steps[k], B, moms[k]), S)
                        tr.sampler.close()
                        n.close()
                    print(json.dumps({
                        "shape": "-".join(map(str, dims)), "dtype": dn, "B": B, "K": K, "iterations": S, "launches_per_step": lpg,
                        "each_us": round(each, 2), "shared_us": round(shared, 2), "lone_us": round(lone, 2),
                        "grouped": grouped, "member_after_member": mixed,
                        "each_over_shared": round(each / shared, 3), "lone_over_each": round(lone / each, 3),
                        "sampler_us_per_batch": round(per_batch[B], 2),
                        "chunk_ms_per_thread": round(per_batch[B] * 256 * ((K + 7) // 8) / 1e3, 3),
                        "chunk_ms_of_steps": round(each * 256 / 1e3, 3)}), flush=True)


if __name__ == "__main__":
    main()
