"""Alternating timings of one KMeans Lloyd step under several dispatch variants.

Usage (on a GPU box):
  python tools/time_kmeans_step.py --n 100000000 --d 128 --k 200 \
      --variants f32,resident --rounds 3 --steps 5

Times `kmeans_assign_reduce` (the loop of tools/bench_baseline_configs.py
km100m) with SRML_KMEANS_VARIANT set to each variant in turn: every variant is
warmed once, then the variants alternate for `--rounds` rounds of `--steps`
synchronised steps each. Prints one JSON line per variant (ms per step: each
round, median, min, max) and one line comparing every variant's results with
the first one's on the same inputs.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spark_rapids_ml_amd.ops import kmeans_assign_reduce  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=100_000_000)
ap.add_argument("--d", type=int, default=128)
ap.add_argument("--k", type=int, default=200)
ap.add_argument("--variants", default="f32,resident")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=5)
args = ap.parse_args()
variants = args.variants.split(",")

assert torch.cuda.is_available(), "needs a GPU"
g = torch.Generator(device="cuda").manual_seed(0)
X = torch.randn(args.n, args.d, generator=g, device="cuda")
C = torch.randn(args.k, args.d, generator=g, device="cuda")
x_sq = (X * X).sum(dim=1)


def step(variant):
    os.environ["SRML_KMEANS_VARIANT"] = variant
    return kmeans_assign_reduce(X, C, x_sq)


results = {}
for v in variants:  # warm-up; the results double as the comparison
    results[v] = step(v)
    torch.cuda.synchronize()

times = {v: [] for v in variants}
for _ in range(args.rounds):
    for v in variants:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step(v)
        torch.cuda.synchronize()
        times[v].append((time.perf_counter() - t0) / args.steps * 1e3)

shape = {"n": args.n, "d": args.d, "k": args.k}
for v in variants:
    t = times[v]
    print(json.dumps({**shape, "variant": v, "ms_per_step": [round(x, 3) for x in t],
                      "median": round(statistics.median(t), 3),
                      "min": round(min(t), 3), "max": round(max(t), 3)}), flush=True)

l0, s0, c0, i0 = results[variants[0]]
for v in variants[1:]:
    l1, s1, c1, i1 = results[v]
    print(json.dumps({**shape, "compare": f"{v} vs {variants[0]}",
                      "labels_equal": float((l0 == l1).float().mean().item()),
                      "sums_max_rel": float(((s0 - s1).abs().max() / s0.abs().max()).item()),
                      "counts_max_abs": float((c0 - c1).abs().max().item()),
                      "inertia_rel": abs(i0 - i1) / abs(i0)}), flush=True)
