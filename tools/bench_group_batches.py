#!/usr/bin/env python3
"""Measurement tool: a NetGroup trained with ONE BATCH SIZE PER MEMBER (NetGroup.train_sampled(samplers, .., batch=[b_0 .. b_{K-1}], ..),
gnn_mlp_group_train_sampled_sizes) on 60 000 synthetic rows.  One JSON line per case, times per iteration of a synchronised run of
--iterations after --warmup:

  case "sweep"   the reference's recorded sweep (logs/trainLog.csv rows 1-3): 784-100-50-10, K = 3, (step, batch) =
                 (0.0042, 2), (0.0075, 4), (0.0100, 8), momentum 0.9
      group_us    the group call: every iteration two grouped launches, member k with its own batch size
      lone_us     the same three runs as lone train_sampled calls one after another: the sum of their times
  case "equal"   784-300-100-10, K = 8, batch 128 for all, one sampler per member
      each_us     through gnn_mlp_group_train_sampled_each: an iteration whose sizes differ at a refill is stepped member after member
      sizes_us    through gnn_mlp_group_train_sampled_sizes: every iteration grouped
      grouped / member_after_member   how each_us's iterations were stepped
Usage: python tools/bench_group_batches.py [--iterations 2000] [--warmup 200] [--dtypes f32,bf16] [--rows 60000] [--repeat 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gnn_amd  # noqa: E402

DTYPES = {"f32": gnn_amd.DTYPE_F32, "bf16": gnn_amd.DTYPE_BF16}
SWEEP = [(0.0042, 2), (0.0075, 4), (0.0100, 8)]


def wall_us(sync, run, iterations):
    sync()
    t0 = time.perf_counter()
    run()
    sync()
    return (time.perf_counter() - t0) / iterations * 1e6


def sweep(pix, lab, dt, S, W):
    dims, N, K = [784, 100, 50, 10], lab.size, len(SWEEP)
    steps, batches, moms = [s for s, _ in SWEEP], [b for _, b in SWEEP], [0.9] * len(SWEEP)
    g = gnn_amd.NetGroup(dims, [1] * K, dtype=dt, max_batch=max(batches))  # (the reference's runs all start from Random(1))
    g.upload_dataset_u8(pix, lab)
    own = [gnn_amd.Sampler(N, seed=1) for _ in range(K)]
    g.train_sampled(own, W, batches, steps, moms)
    group = wall_us(g.synchronize, lambda: g.train_sampled(own, S, batches, steps, moms), S)
    counts = g.sampled_each_iterations
    for x in own + [g]:
        x.close()
    lone = 0.0
    for k in range(K):
        n = gnn_amd.SoftmaxCrossEntropyNeuralNet(dims, seed=1, dtype=dt, max_batch=max(batches))
        tr = gnn_amd.NeuralNetTrainer(pix, lab, n, raw_u8=True, seed=1)
        tr.train(W, steps[k], batches[k], moms[k])
        lone += wall_us(n.synchronize, lambda: tr.train(S, steps[k], batches[k], moms[k]), S)
        tr.sampler.close()
        n.close()
    return {"case": "sweep", "shape": "-".join(map(str, dims)), "K": K, "batches": batches, "group_us": round(group, 2),
            "lone_us": round(lone, 2), "lone_over_group": round(lone / group, 3), "grouped": counts[0], "member_after_member": counts[1]}


def equal(pix, lab, dt, S, W):
    dims, N, K, B = [784, 300, 100, 10], lab.size, 8, 128
    steps, moms = [0.0125 * (1 + 0.1 * k) for k in range(K)], [0.9] * K
    out = {"case": "equal", "shape": "-".join(map(str, dims)), "K": K, "B": B}
    for key, batch in (("each_us", B), ("sizes_us", [B] * K)):
        g = gnn_amd.NetGroup(dims, list(range(1, K + 1)), dtype=dt, max_batch=B)
        g.upload_dataset_u8(pix, lab)
        own = [gnn_amd.Sampler(N, seed=k + 1) for k in range(K)]
        g.train_sampled(own, W, batch, steps, moms)
        out[key] = round(wall_us(g.synchronize, lambda: g.train_sampled(own, S, batch, steps, moms), S), 2)
        if key == "each_us":
            out["grouped"], out["member_after_member"] = g.sampled_each_iterations
        for x in own + [g]:
            x.close()
    out["each_over_sizes"] = round(out["each_us"] / out["sizes_us"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--dtypes", default="f32,bf16")
    ap.add_argument("--rows", type=int, default=60000)
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    pix = rng.integers(0, 256, (a.rows, 784), dtype=np.uint8)
    lab = rng.integers(0, 10, a.rows, dtype=np.uint8)
    for dn in a.dtypes.split(","):
        for case in (sweep, equal):
            for r in range(a.repeat):
                line = case(pix, lab, DTYPES[dn], a.iterations, a.warmup)
                line.update({"dtype": dn, "iterations": a.iterations, "run": r})
                print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
