"""Flagship benchmark: distributed KMeans fit on synthetic 1M×3000 f32/GPU.

Measures the reference's headline workload (KMeans k=1000,
maxIter=30 on 1M×3000 float32 — the 116× speedup row) as steady-state Lloyd
iterations/s. A "step" is one full Lloyd iteration: fused MFMA
distance+argmin kernel, per-center sum/count accumulation, ONE fused RCCL
all-reduce of [k×(d+2)] over xGMI, centroid update. Weak scaling: each of
the N ranks holds its own 1M×3000 shard.

Launch (driver contract):
  python bench.py --gpus 1 --steps K --warmup W
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
      --master-addr 127.0.0.1 bench.py --gpus N --steps K --warmup W

A plain run sets up, warms up, times the K steps and prints the result line.
  --full              also times the whole-job fit() (host->device ingest +
                      init + 30 Lloyd iterations) and reports `fit_wall_s`,
                      `fit_rows_per_s` and the whole-job `vs_baseline`
  --dump-outputs DIR  write what the last timed step returned (centers,
                      labels, counts, inertia) as DIR/<name>.npy
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import torch

# Reference baseline: 1M rows × 30 Lloyd iterations in 82 s
# fit wall-clock on 2×A10G => 365,854 row-iterations/s whole-job.
BASELINE_ROWS_PER_S = 1_000_000 * 30 / 82.0


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, default=None, help="rows per GPU")
    ap.add_argument("--cols", type=int, default=3000)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--full", action="store_true",
                    help="also time the whole-job fit() against the reference's 82 s")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs as DIR/<name>.npy")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be >= 1")

    from spark_rapids_ml_amd.parallel.context import get_comm, init_comm, shutdown_comm
    from spark_rapids_ml_amd.ops import kmeans_assign_reduce

    comm = init_comm()
    on_gpu = comm.device.type == "cuda"
    rows = args.rows if args.rows is not None else (1_000_000 if on_gpu else 20_000)
    cols = args.cols if on_gpu else min(args.cols, 256)
    k = args.k if on_gpu else min(args.k, 64)

    dev = comm.device
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234 + comm.rank)
    # synthetic blob-ish data: k latent centers + noise, generated on-device
    latent = torch.randn(k, cols, generator=gen, device=dev, dtype=torch.float32)
    X = torch.empty(rows, cols, device=dev, dtype=torch.float32)
    chunk = 1 << 18
    for s in range(0, rows, chunk):
        e = min(rows, s + chunk)
        assign = torch.randint(0, k, (e - s,), generator=gen, device=dev)
        X[s:e] = latent[assign] + 0.5 * torch.randn(e - s, cols, generator=gen, device=dev)
    x_sq = (X * X).sum(dim=1)

    # random-init centers, identical on all ranks
    g0 = torch.Generator(device=dev)
    g0.manual_seed(42)
    C = torch.randn(k, cols, generator=g0, device=dev, dtype=torch.float32)

    last = {}  # what the most recent step handed back (for --dump-outputs)

    def lloyd_step(C: torch.Tensor) -> torch.Tensor:
        labels, sums, counts, inertia = kmeans_assign_reduce(X, C, x_sq)
        buf = torch.empty((k, cols + 2), dtype=torch.float64, device=sums.device)
        buf[:, :cols] = sums
        buf[:, cols] = counts
        buf[0, cols + 1] = inertia
        buf = comm.allreduce_t(buf)
        g_counts = buf[:, cols]
        nonempty = g_counts > 0
        C_new = C.clone()
        C_new[nonempty] = (buf[nonempty, :cols] / g_counts[nonempty, None]).to(C.dtype)
        last.update(labels=labels, counts=g_counts, inertia=buf[0, cols + 1])
        return C_new

    for _ in range(args.warmup):
        C = lloyd_step(C)

    comm.barrier()
    if on_gpu:
        torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        C = lloyd_step(C)
    if on_gpu:
        torch.cuda.synchronize(dev)
    comm.barrier()
    elapsed = time.perf_counter() - t0
    elapsed = comm.allreduce_scalar(elapsed, "max")

    n_gpus = comm.world_size
    total_rows = rows * n_gpus
    value = total_rows * args.steps / elapsed
    ms_per_step = elapsed / args.steps * 1000.0

    if args.dump_outputs and comm.rank == 0:
        # 1000×3000 f32 centers + 1M labels ≈ 16 MB at the default shape
        os.makedirs(args.dump_outputs, exist_ok=True)
        for name, t, dt in (
            ("centers", C, np.float32),
            ("labels", last["labels"], np.float32),  # ids < k: exact in f32
            ("counts", last["counts"], np.float64),
            ("inertia", last["inertia"].reshape(1), np.float64),
        ):
            np.save(os.path.join(args.dump_outputs, name + ".npy"),
                    t.detach().cpu().numpy().astype(dt))

    fit_iters = 30 if on_gpu else 5
    full = {}
    if args.full:
        # Whole-job fit wall-clock (the honest vs-baseline basis):
        # host→device ingest + k init + 30 Lloyd iterations through the real
        # estimator path, exactly the job the reference's 82 s covers.
        from spark_rapids_ml_amd import KMeans as _KMeans
        from spark_rapids_ml_amd.data import DataFrame as _DF

        Xh = X.cpu().numpy()
        del X, x_sq
        if on_gpu:
            torch.cuda.empty_cache()
        comm.barrier()
        t0 = time.perf_counter()
        _KMeans(k=k, maxIter=fit_iters, initMode="random", seed=5).fit(_DF.from_numpy(Xh))
        if on_gpu:
            torch.cuda.synchronize(dev)
        comm.barrier()
        fit_wall_s = comm.allreduce_scalar(time.perf_counter() - t0, "max")
        fit_rows_per_s = total_rows * fit_iters / fit_wall_s
        full = {
            # whole-job ÷ whole-job: full fit() wall-clock (ingest+init+30
            # Lloyd iters) vs the reference's published 82 s on the same
            # 1M×3000 k=1000 workload — NOT the steady-state step rate
            "vs_baseline": fit_rows_per_s / BASELINE_ROWS_PER_S if on_gpu else None,
            "fit_wall_s": fit_wall_s,
            "fit_rows_per_s": fit_rows_per_s,
        }

    if comm.rank == 0:
        out = {
            "metric": "kmeans_fit_rows_per_s",
            "value": value,
            "unit": "row-iterations/s",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "weak",
            **full,
            "steady_state_vs_baseline": value / BASELINE_ROWS_PER_S if on_gpu else None,
            "dtype": "fp32",
            "data": "synthetic",
            "config": {
                "model": "KMeans k=1000 (BASELINE.md headline: 116x row)",
                "rows_per_gpu": rows,
                "cols": cols,
                "k": k,
                "maxIter_full_fit": fit_iters,
                "global_batch": total_rows,
                "seq_len": None,
                "parallelism": f"dp{n_gpus}",
            },
        }
        print(json.dumps(out))
    shutdown_comm()


if __name__ == "__main__":
    main()
