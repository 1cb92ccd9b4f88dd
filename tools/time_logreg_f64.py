"""Alternating timings of one f64 `logistic_grad_loss` call: the f64 MFMA
kernels against the expressions they replace.

Usage (on a GPU box):
  python tools/time_logreg_f64.py --n 1000000 --d 128 --classes 10 --rounds 5 --steps 5

Times `logistic_grad_loss` on f64 device tensors (`logreg_grad_loss_f64`) and,
on the same tensors, what f64 rows ran before that kernel existed, kept
callable only here: a torch f64 GEMM for the scores, the f32
`softmax_residual_loss` kernel, and a second torch f64 GEMM. Both are warmed
once, then alternated for `--rounds` rounds of `--steps` synchronised calls
(host clock around a device synchronise). Prints one JSON line per timed thing
with median, min and max, the rate at which the new path reads X (it reads it
twice), and one line comparing the two results. The kernels' own times come
from a profiler: `--steps 1 --rounds 1 --no-old` is the run to put under it.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spark_rapids_ml_amd.ops.dispatch import hip_ops  # noqa: E402
from spark_rapids_ml_amd.ops.glm import logistic_grad_loss  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--d", type=int, default=128)
ap.add_argument("--classes", type=int, default=10, help="rows of W; 1 is the sigmoid")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--no-old", action="store_true")
args = ap.parse_args()

assert torch.cuda.is_available(), "needs a GPU"
ext = hip_ops()
g = torch.Generator(device="cuda").manual_seed(0)
n, d, C = args.n, args.d, args.classes
X = torch.empty(n, d, device="cuda", dtype=torch.float64)
for s in range(0, n, 1 << 16):
    X[s:s + (1 << 16)].normal_(generator=g)
W = torch.randn(C, d + 1, generator=g, device="cuda", dtype=torch.float64) / d ** 0.5
y = torch.randint(0, max(C, 2), (n,), generator=g, device="cuda")


def old_path():
    scores = X @ W[:, :d].T + W[:, d][None, :]
    resid, loss = ext.softmax_residual_loss(scores.contiguous().to(torch.float32), y)
    resid = resid.to(torch.float64)
    return torch.cat([resid.T @ X, resid.sum(dim=0)[:, None]], dim=1), loss


things = {"new": lambda: logistic_grad_loss(X, y, W, True)}
if not args.no_old:
    things["old"] = old_path

results = {}
for name, fn in things.items():
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

shape = {"n": n, "d": d, "classes": C}
for name, t in times.items():
    med = statistics.median(t)
    line = {**shape, "timed": name, "ms": [round(x, 3) for x in t],
            "median": round(med, 3), "min": round(min(t), 3), "max": round(max(t), 3)}
    if name == "new":
        line["x_tb_per_s"] = round(2 * n * d * 8 / (med * 1e-3) / 1e12, 2)
    print(json.dumps(line), flush=True)

if "old" in results:
    (g0, l0), (g1, l1) = results["new"], results["old"]
    print(json.dumps({**shape, "compare": "old vs new",
                      "grad_max_rel": float(((g0 - g1).abs().max() / g0.abs().max()).item()),
                      "loss_rel": abs(float(l0) - float(l1)) / abs(float(l0))}), flush=True)
