"""Time the wide selection kernel (64 < k <= 1024) against the torch path it
replaces, alternating SRML_KNN_KERNEL=0 and the default in ONE process.

Usage:
  python tools/time_knn_wide.py                       # every case below
  python tools/time_knn_wide.py --cases self --ks 1024 --factors 8,16,32

Cases: `bench` is `knn_topk` at the exact-kNN bench's default shape
(benchmark_runner.py nearest_neighbors: 10 000 queries against 100 000 x 300
blobs); `self` a UMAP-like self-kNN of 100 000 x 64; `tile` manhattan and
`sparse` jaccard at k = 128; `many` (not in the default set) 1 000 000
queries against 100 000 x 64, where the query tiling decides the chunk width. Each setting is warmed up once, then the two
alternate for --repeats rounds; a timed window is --inner calls and ends in
a device synchronise. The tile and sparse dispatchers have no environment
switch, so their torch side calls `torch_ref` directly. The neighbour sets of the last round are compared: sorted keys up to
f32 reordering, and ids that only one path names must sit at the row's k-th
key (a tie). --factors re-times the kernel path under each WIDE_CHUNK_FACTOR.
Prints one JSON line per case and k.
"""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402
import torch  # noqa: E402

from benchmark import gen_data  # noqa: E402
from spark_rapids_ml_amd.ops import knn as knn_ops  # noqa: E402
from spark_rapids_ml_amd.ops import torch_ref  # noqa: E402


def _stats(ts):
    a = np.asarray(ts)
    return {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max()),
            "all": [round(float(v), 4) for v in a]}


def _timed(fn, inner):
    """Seconds per call over a window of `inner` calls, and the last result."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner, out


def _compare(torch_out, kernel_out, block=4096):
    """Largest relative gap of the sorted keys, rows whose id sets differ, and
    how far (relative) an id named by one path only sits from the k-th key."""
    (dt, it), (dk, ik) = torch_out, kernel_out
    k = dt.shape[1]
    scale = dt[:, -1:].abs().clamp(min=1e-30)
    key_gap = ((dt - dk).abs() / scale).max().item()
    # euclidean keys are roots: a self-distance is the root of pure rounding
    # error, so the squared keys are compared as well
    sq_gap = ((dt * dt - dk * dk).abs() / (scale * scale)).max().item()
    rows_differ, tie_gap = 0, 0.0
    for s in range(0, dt.shape[0], block):
        ids = torch.cat([it[s:s + block], ik[s:s + block]], dim=1)
        keys = torch.cat([dt[s:s + block], dk[s:s + block]], dim=1)
        ids, order = torch.sort(ids, dim=1)
        keys = keys.gather(1, order)
        pad = torch.full_like(ids[:, :1], -2)
        once = (ids != torch.cat([pad, ids[:, :-1]], 1)) & (ids != torch.cat([ids[:, 1:], pad], 1))
        rows_differ += int(once.any(dim=1).sum())
        kth = torch.maximum(dt[s:s + block, -1:], dk[s:s + block, -1:])
        gap = ((keys - kth).abs() / scale[s:s + block])[once]
        tie_gap = max(tie_gap, gap.max().item() if gap.numel() else 0.0)
    return {"k": k, "max_rel_key_gap": key_gap, "max_rel_squared_key_gap": sq_gap,
            "rows_with_other_ids": rows_differ,
            "max_rel_gap_of_other_ids_to_kth_key": tie_gap}


def _run_case(name, k, call, args, factors):
    default_factor = knn_ops.WIDE_CHUNK_FACTOR

    def run(setting, factor=None):
        # the env switch is knn_topk's; the other two dispatchers have none,
        # so their cases call torch_ref themselves when `kernel` is False
        if setting == "0":
            os.environ["SRML_KNN_KERNEL"] = "0"
        else:
            os.environ.pop("SRML_KNN_KERNEL", None)
        knn_ops.WIDE_CHUNK_FACTOR = factor or default_factor
        return call(k, setting != "0")

    settings = [("0", None), ("default", None)] + [("default", f) for f in factors]
    if args.kernel_only:
        settings = settings[1:]
    times = {s: [] for s in settings}
    out = {}
    for s in settings:  # warm-up
        run(*s)
    for _ in range(args.repeats):
        for s in settings:
            t, out[s] = _timed(lambda: run(*s), args.inner)
            times[s].append(t)
    knn_ops.WIDE_CHUNK_FACTOR = default_factor
    report = {"case": name, "k": k}
    for s in settings:
        name_s = "torch_sec" if s[0] == "0" else "kernel_sec" + (f"[factor={s[1]}]" if s[1] else "")
        report[name_s] = _stats(times[s])
    if not args.kernel_only:
        report["speedup_median"] = report["torch_sec"]["median"] / report["kernel_sec"]["median"]
        report.update(_compare(out[settings[0]], out[settings[1]]))
    os.environ.pop("SRML_KNN_KERNEL", None)
    print(json.dumps(report), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="bench,self,tile,sparse")
    ap.add_argument("--ks", default="65,128,256,1024")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed window")
    ap.add_argument("--kernel_only", action="store_true", help="skip the torch path (profiling)")
    ap.add_argument("--factors", default="", help="comma list of WIDE_CHUNK_FACTOR values")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_knn_wide.py measures on the GPU"
    cases = args.cases.split(",")
    ks = [int(v) for v in args.ks.split(",")]
    factors = [int(v) for v in args.factors.split(",") if v]
    dev = torch.device("cuda")

    def dense(rows, cols):
        X, _ = gen_data.gen_blobs(rows, cols, seed=0)
        return torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).to(dev)

    if "bench" in cases:
        I = dense(100000, 300)
        Q = I[:10000].contiguous()
        for k in ks:
            _run_case("bench 10000 x 100000 x 300 euclidean", k,
                      lambda k, kernel: knn_ops.knn_topk(Q, I, k), args, factors)
    if "self" in cases:
        X = dense(100000, 64)
        for k in ks:
            _run_case("self 100000 x 64 euclidean", k,
                      lambda k, kernel: knn_ops.knn_topk(X, X, k), args, factors)
    if "many" in cases:  # state traffic: 1M queries leave narrow item chunks
        I = dense(100000, 64)
        Q = I.repeat(10, 1)
        for k in ks:
            _run_case("many 1000000 x 100000 x 64 euclidean", k,
                      lambda k, kernel: knn_ops.knn_topk(Q, I, k), args, factors)
    if "tile" in cases:
        I = dense(100000, 32)
        Q = I[:10000].contiguous()
        _run_case("tile 10000 x 100000 x 32 manhattan", 128,
                  lambda k, kernel: knn_ops.knn_topk_metric(Q, I, k, "manhattan") if kernel
                  else torch_ref.knn_topk_metric(Q, I, k, "manhattan", 2.0), args, [])
    if "sparse" in cases:
        M = sp.random(50000, 1000, density=0.02, format="csr", dtype=np.float32,
                      random_state=np.random.default_rng(0))
        M = knn_ops.canonical_csr(M)
        Qs = knn_ops.canonical_csr(M[:5000])
        _run_case("sparse 5000 x 50000 x 1000 (2 %) jaccard", 128,
                  lambda k, kernel: knn_ops.knn_topk_metric_sparse(Qs, M, k, "jaccard", device=dev)
                  if kernel else torch_ref.knn_topk_metric_sparse(Qs, M, k, "jaccard", 2.0, dev),
                  args, [])


if __name__ == "__main__":
    main()
