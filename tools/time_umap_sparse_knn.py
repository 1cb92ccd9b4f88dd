"""Time UMAP's sparse kNN-graph stage against the densified one on the GPU.

Usage: python tools/time_umap_sparse_knn.py [--n 20000] [--d 20000]
           [--density 0.005] [--k 16] [--reps 3] [--profile]

For manhattan and cosine: `knn_topk_metric_sparse(X, X, k)` at item chunks of
8192 and 4096 (one and two `csr_pairwise` blocks per CU) and the baseline
`knn_topk_metric` on the densified tensor, alternated `reps` times after one
warm-up each, a device synchronise inside every timed window. The host-side
canonicalisation and upload of the CSR is part of the sparse time; the
densified tensor is uploaded once outside the baseline's. Also prints how many
rows' neighbour sets differ between the two paths. `--profile` runs each sparse
variant once and nothing else, for a kernel trace. One JSON line per result.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from spark_rapids_ml_amd.ops.knn import (  # noqa: E402
    _sparse_rows,
    canonical_csr,
    knn_topk_metric,
    knn_topk_metric_sparse,
)


def make(n: int, d: int, density: float) -> sp.csr_matrix:
    rng = np.random.default_rng(0)
    X = sp.random(n, d, density=density, random_state=rng,
                  data_rvs=lambda m: rng.gamma(2.0, 1.0, m).astype(np.float32))
    # one more entry per row: no zero rows under cosine
    X = X + sp.csr_matrix((np.ones(n, np.float32), (np.arange(n), np.arange(n) % d)), shape=(n, d))
    return X.tocsr().astype(np.float32)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--d", type=int, default=20000)
    ap.add_argument("--density", type=float, default=0.005)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"

    X = make(a.n, a.d, a.density)
    shape = {"n": a.n, "d": a.d, "density": a.density, "nnz": int(X.nnz), "k": a.k}
    for metric in ("manhattan", "cosine"):
        variants = {
            "sparse_c8192": lambda: knn_topk_metric_sparse(X, X, a.k, metric, device="cuda", chunk=8192),
            "sparse_c4096": lambda: knn_topk_metric_sparse(X, X, a.k, metric, device="cuda", chunk=4096),
        }
        if a.profile:
            for fn in variants.values():
                timed(fn)
            continue
        Xd = torch.from_numpy(X.toarray()).cuda()
        variants["dense"] = lambda: knn_topk_metric(Xd, Xd, a.k, metric)
        times = {name: [] for name in variants}
        outs = {}
        for name, fn in variants.items():  # warm-up
            outs[name] = timed(fn)[1]
        for _ in range(a.reps):
            for name, fn in variants.items():
                times[name].append(timed(fn)[0])
        # the host share of a sparse call: canonicalisation + row constants
        host = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            _sparse_rows(canonical_csr(X), metric, 2.0)
            host.append(round((time.perf_counter() - t0) * 1e3, 2))
        print(json.dumps({"metric": metric, "variant": "host_prep_only", "ms": host}), flush=True)
        ref = torch.sort(outs["dense"][1], dim=1)[0]
        for name in variants:
            diff = int((torch.sort(outs[name][1], dim=1)[0] != ref).any(dim=1).sum())
            print(json.dumps({
                "metric": metric, "variant": name, **shape,
                "ms": [round(t, 2) for t in times[name]], "ms_min": round(min(times[name]), 2),
                "rows_differing_from_dense": diff,
            }), flush=True)
        del Xd


if __name__ == "__main__":
    main()
