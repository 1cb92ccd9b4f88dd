"""Alternating timings of the f64 moment set: `moments_f64` against torch.

Usage (on a GPU box):
  python tools/time_moments_f64.py            # the three shapes, then the fits
  python tools/time_moments_f64.py --profile  # 3 kernel calls a shape, nothing else

Times `ops.linalg.moments(X, y)` on f64 device tensors (the `moments_f64`
kernel) and the five torch expressions it replaced (`X.T @ X`, `X.sum(0)`,
`X.T @ y`, `y.sum()`, `(y * y).sum()`) on the same tensors: both warmed twice,
then alternated, each call between two device events. Then the wall clock of
`PCA(k=3)` and `LinearRegression()` with `float32_inputs=False` on host rows,
with the kernel and with SRML_MOMENTS_F64=0, alternated, the first of each
dropped. Prints one JSON line per timed thing. `--profile` is the run to put
under `rocprofv3 --kernel-trace --stats`.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spark_rapids_ml_amd.ops.linalg import moments  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--profile", action="store_true")
ap.add_argument("--fit_rows", type=int, default=1_000_000)
ap.add_argument("--fit_cols", type=int, default=512)
args = ap.parse_args()
SHAPES = ((1_000_000, 128, 12), (1_000_000, 512, 8), (1_000_000, 3000, 4))


def parent(X, y):
    G = (X.T @ X).to(torch.float64)
    xs = X.sum(dim=0).to(torch.float64)
    xy = (X.T @ y).to(torch.float64)
    return G, xs, xy, y.sum().to(torch.float64), (y * y).sum().to(torch.float64)


def timed(fn, *a):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn(*a)
    e.record()
    e.synchronize()
    return s.elapsed_time(e), out


for n, d, reps in SHAPES:
    torch.manual_seed(0)
    X = torch.randn(n, d, dtype=torch.float64, device="cuda") + 3.0
    y = torch.randn(n, dtype=torch.float64, device="cuda")
    if args.profile:
        for _ in range(3):
            moments(X, y)
        torch.cuda.synchronize()
    else:
        for _ in range(2):
            timed(moments, X, y)
            timed(parent, X, y)
        tn, tp = [], []
        for _ in range(reps):
            a, new = timed(moments, X, y)
            b, old = timed(parent, X, y)
            tn.append(round(a, 3))
            tp.append(round(b, 3))
        rel = max(float((p - q).abs().max() / q.abs().max()) for p, q in zip(new, old))
        da = d + 2
        print(json.dumps({
            "shape": [n, d], "kernel_ms": tn, "torch_ms": tp,
            "kernel_median_ms": statistics.median(tn), "torch_median_ms": statistics.median(tp),
            "max_rel_diff": rel,
            "upper_triangle_flop": n * da * (da + 128),  # 2 per FMA over the 128-wide tiles
        }), flush=True)
        del new, old
    del X, y
    torch.cuda.empty_cache()

if not args.profile:
    from spark_rapids_ml_amd import PCA, LinearRegression  # noqa: E402
    from spark_rapids_ml_amd.data import DataFrame  # noqa: E402

    rng = np.random.default_rng(0)
    X = rng.standard_normal((args.fit_rows, args.fit_cols)) + 3.0
    y = X[:, :8].sum(1) + rng.standard_normal(args.fit_rows)
    dfx, dfxy = DataFrame.from_numpy(X), DataFrame.from_numpy(X, y)
    fits = {"PCA(k=3)": lambda: PCA(k=3, float32_inputs=False).fit(dfx),
            "LinearRegression()": lambda: LinearRegression(float32_inputs=False).fit(dfxy)}
    for name, fit in fits.items():
        t = {"1": [], "0": []}
        for rep in range(4):
            for sw in ("1", "0"):
                os.environ["SRML_MOMENTS_F64"] = sw
                t0 = time.perf_counter()
                fit()
                torch.cuda.synchronize()
                if rep:
                    t[sw].append(round(time.perf_counter() - t0, 4))
        print(json.dumps({"fit": name, "shape": [args.fit_rows, args.fit_cols],
                          "kernel_s": t["1"], "torch_s": t["0"]}), flush=True)
