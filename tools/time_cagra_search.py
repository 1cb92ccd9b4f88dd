"""Time the CAGRA graph search and the index cache at the ANN bench's default
shape (benchmark_runner.py approximate_nearest_neighbors --algorithm cagra),
in ONE process.

Usage:
  python tools/time_cagra_search.py
  python tools/time_cagra_search.py --kernel_only --skip_kneighbors   # profiler run

Search alone: the graph is built once, then SRML_CAGRA_KERNEL=0 (torch beam
search, the search code from before the kernel) and =1 (`cagra_search`
kernel) alternate for --repeats rounds after one warm-up each, with a device
synchronise inside the timed window. Both paths' recall@k is judged against
the exact NearestNeighbors, and the kernel's per-query stats are averaged.

Whole kneighbors: per round a fresh model's first call (build + query) and
its second call (query on the kept index) under the default setting.
Prints one JSON line.
"""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from benchmark import gen_data  # noqa: E402
from spark_rapids_ml_amd import ApproximateNearestNeighbors, NearestNeighbors  # noqa: E402
from spark_rapids_ml_amd.data import DataFrame  # noqa: E402
from spark_rapids_ml_amd.models import knn as knn_mod  # noqa: E402
from spark_rapids_ml_amd.parallel.context import get_comm, init_comm  # noqa: E402


def _sync():
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def _stats(ts):
    a = np.asarray(ts)
    return {
        "median": float(np.median(a)), "min": float(a.min()), "max": float(a.max()),
        "all": [round(float(v), 4) for v in a],
    }


def _set_env(s):
    if s == "default":
        os.environ.pop("SRML_CAGRA_KERNEL", None)
    else:
        os.environ["SRML_CAGRA_KERNEL"] = s


def _recall(found, truth):
    hits = sum(len(set(a.tolist()) & set(b.tolist())) for a, b in zip(found, truth))
    return hits / truth.size


def main() -> None:
    ap = argparse.ArgumentParser()
    # defaults = benchmark_runner.py approximate_nearest_neighbors defaults
    ap.add_argument("--num_rows", type=int, default=100000)
    ap.add_argument("--num_cols", type=int, default=300)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--num_queries", type=int, default=10000)
    ap.add_argument("--graph_degree", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip_kneighbors", action="store_true")
    ap.add_argument("--kernel_only", action="store_true",
                    help="skip the torch search and the recall (for a profiler run)")
    ap.add_argument("--rehearse", action="store_true",
                    help="run without the kernel (no GPU): checks the script, times nothing real")
    args = ap.parse_args()

    init_comm()
    dev = get_comm().device
    X, _ = gen_data.gen_blobs(args.num_rows, args.num_cols, seed=0)
    params = {"graph_degree": args.graph_degree}
    nq = min(args.num_queries, X.shape[0])
    itopk, width, max_it = knn_mod._cagra_search_params(params, args.k)
    report = {"num_rows": args.num_rows, "num_cols": args.num_cols, "k": args.k,
              "num_queries": nq, "graph_degree": args.graph_degree, "itopk_size": itopk,
              "search_width": width, "max_iterations": max_it}

    # -- search alone, graph built once ---------------------------------------
    Xt = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).to(dev)
    _sync()
    t0 = time.perf_counter()
    index = knn_mod._cagra_build(Xt, params)
    _sync()
    report["build_sec"] = round(time.perf_counter() - t0, 4)
    report["search_graph_degree"] = int(index.G.shape[1])
    Qt = Xt[:nq].contiguous()

    names = {"1": "kernel"} if args.kernel_only else {"0": "torch", "1": "kernel"}
    times = {s: [] for s in names}
    out = {}
    for s in names:  # warm-up
        _set_env(s)
        report[f"kernel_path[SRML_CAGRA_KERNEL={s}]"] = bool(
            knn_mod._cagra_kernel_wanted(index, Qt, args.k, itopk, width)
        )
        knn_mod._cagra_query(index, Qt, args.k, itopk, width, max_it)
    if not report["kernel_path[SRML_CAGRA_KERNEL=1]"] and not args.rehearse:
        raise SystemExit("the cagra_search kernel is not available here: nothing to time")
    for _ in range(args.repeats):
        for s in names:
            _set_env(s)
            _sync()
            t0 = time.perf_counter()
            out[s] = knn_mod._cagra_query(index, Qt, args.k, itopk, width, max_it)
            _sync()
            times[s].append(time.perf_counter() - t0)
    for s, name in names.items():
        report[f"search_only_sec[{name}]"] = _stats(times[s])
    if report["kernel_path[SRML_CAGRA_KERNEL=1]"]:
        _, _, st = knn_mod._cagra_search_kernel(index, Qt, args.k, itopk, width, max_it)
        report["mean_stats_per_query[iterations, evaluations, resets]"] = [
            round(float(v), 2) for v in st.double().mean(dim=0).tolist()
        ]
    if len(names) == 2:
        report["torch_fastest_over_kernel_median"] = (
            report["search_only_sec[torch]"]["min"] / report["search_only_sec[kernel]"]["median"]
        )
        df = DataFrame.from_numpy(X)
        exact = NearestNeighbors(k=args.k).fit(df)
        _, _, res = exact.kneighbors(df.take_local(np.arange(nq)))
        truth = np.asarray(res["indices"])
        for s, name in names.items():
            report[f"recall@{args.k}[{name}]"] = _recall(out[s][1].cpu().numpy(), truth)
    del out

    # -- whole kneighbors: first call (build + query) against second ---------
    if not args.skip_kneighbors:
        _set_env("default")
        df = DataFrame.from_numpy(X)
        q = df.take_local(np.arange(nq))
        first, second = [], []
        for r in range(args.repeats + 1):  # round 0 is the warm-up
            model = ApproximateNearestNeighbors(
                k=args.k, algorithm="cagra", algoParams=params,
            ).fit(df)
            for sink in (first, second):
                _sync()
                t0 = time.perf_counter()
                model.kneighbors(q)
                _sync()
                if r:
                    sink.append(time.perf_counter() - t0)
        report["kneighbors_first_call_sec"] = _stats(first)
        report["kneighbors_second_call_sec"] = _stats(second)

    print(json.dumps(report))


if __name__ == "__main__":
    main()
