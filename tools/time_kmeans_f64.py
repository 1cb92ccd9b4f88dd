"""Alternating timings of one f64 KMeans Lloyd step: HIP kernels against torch.

Usage (on a GPU box):
  python tools/time_kmeans_f64.py --n 1000000 --d 3000 --k 1000 --rounds 5 --steps 5

Times `kmeans_assign_reduce` on f64 device tensors (`kmeans_assign_f64` +
`label_accumulate_f64`) and `torch_ref.kmeans_assign_reduce` on the same
tensors: both warmed once, then alternated for `--rounds` rounds of `--steps`
synchronised steps each (host clock around a device synchronise). The two
extension calls are timed the same way on their own, with the rates that
follow from the shape: 2·n·k·d FLOP for the assign call, n·d·8 bytes of rows
for the accumulation. Prints one JSON line per timed thing and one comparing
the two paths' results. `--steps 1 --rounds 1 --no-torch` is the run to put
under a profiler.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spark_rapids_ml_amd.ops import kmeans_assign_reduce, torch_ref  # noqa: E402
from spark_rapids_ml_amd.ops.dispatch import hip_ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--d", type=int, default=3000)
ap.add_argument("--k", type=int, default=1000)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--no-torch", action="store_true")
args = ap.parse_args()

assert torch.cuda.is_available(), "needs a GPU"
ext = hip_ops()
g = torch.Generator(device="cuda").manual_seed(0)
n, d, k = args.n, args.d, args.k
C = torch.randn(k, d, generator=g, device="cuda", dtype=torch.float64)
X = torch.empty(n, d, device="cuda", dtype=torch.float64)
for s in range(0, n, 1 << 16):  # rows near centres, so the labels are decided
    e = min(n, s + (1 << 16))
    own = torch.randint(0, k, (e - s,), generator=g, device="cuda")
    X[s:e] = C[own] + 0.5 * torch.randn(e - s, d, generator=g, device="cuda", dtype=torch.float64)
C = C + 0.05 * torch.randn(k, d, generator=g, device="cuda", dtype=torch.float64)
x_sq = (X * X).sum(dim=1)
labels0 = ext.kmeans_assign_f64(X, C, x_sq)[0]

things = {
    "hip": lambda: kmeans_assign_reduce(X, C, x_sq),
    "kmeans_assign_f64": lambda: ext.kmeans_assign_f64(X, C, x_sq),
    "label_accumulate_f64": lambda: ext.label_accumulate_f64(X, labels0, k),
}
if not args.no_torch:
    things["torch"] = lambda: torch_ref.kmeans_assign_reduce(X, C, x_sq)

results = {}
for name, fn in things.items():  # warm-up; the results double as the comparison
    results[name] = fn()
    torch.cuda.synchronize()

times = {name: [] for name in things}
for _ in range(args.rounds):
    for name, fn in things.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize()
        times[name].append((time.perf_counter() - t0) / args.steps * 1e3)

shape = {"n": n, "d": d, "k": k}
for name, t in times.items():
    med = statistics.median(t)
    line = {**shape, "timed": name, "ms": [round(x, 3) for x in t],
            "median": round(med, 3), "min": round(min(t), 3), "max": round(max(t), 3)}
    if name == "kmeans_assign_f64":
        line["tflops_f64"] = round(2.0 * n * k * d / (med * 1e-3) / 1e12, 2)
    if name == "label_accumulate_f64":
        line["row_gb_per_s"] = round(n * d * 8 / (med * 1e-3) / 1e9, 1)
    print(json.dumps(line), flush=True)

if "torch" in results:
    (l0, s0, c0, i0), (l1, s1, c1, i1) = results["hip"], results["torch"]
    print(json.dumps({**shape, "compare": "torch vs hip",
                      "labels_equal": float((l0 == l1).double().mean().item()),
                      "sums_max_rel": float(((s0 - s1).abs().max() / s0.abs().max()).item()),
                      "counts_max_abs": float((c0 - c1).abs().max().item()),
                      "inertia_rel": abs(i0 - i1) / abs(i0)}), flush=True)
