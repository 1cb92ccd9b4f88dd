"""Time the CAGRA builds and search their graphs at the ANN bench's default
shape (benchmark_runner.py approximate_nearest_neighbors --algorithm cagra),
in ONE process.

Usage:
  python tools/time_cagra_build.py
  python tools/time_cagra_build.py --prune_only          # profiler run
  python tools/time_cagra_build.py --rehearse --num_rows 3000 --num_cols 16 \
      --num_queries 200                                  # no GPU: checks the script

Builds: the default build (graph_degree forward + graph_degree // 2 reverse
columns) against the optimised builds --configs (intermediate:graph_degree),
the latter split into the intermediate kNN graph, the pruning (`cagra_prune`
kernel and, with SRML_CAGRA_PRUNE_KERNEL=0, the torch formulation on the same
device) and the reverse-edge merge. One warm-up, then --repeats rounds, a
device synchronise inside every timed window. The pruning is also reported as
GB/s of its n * D rows of 4 * D bytes gathered.

Search: every graph under the default search parameters for k: seconds,
recall@k against the exact NearestNeighbors, and the rows keyed per query
(the kernel's stats[:, 1]). The ivf_pq build (first of --configs) is built,
timed and searched the same way.
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
from spark_rapids_ml_amd import NearestNeighbors  # noqa: E402
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
        "all": [round(float(v), 5) for v in a],
    }


def _timed(fn, repeats, what=""):
    """(last result, seconds of `repeats` rounds after one warm-up)."""
    print(f"timing {what} ...", file=sys.stderr, flush=True)
    out = fn()
    ts = []
    for _ in range(repeats):
        _sync()
        t0 = time.perf_counter()
        out = fn()
        _sync()
        ts.append(time.perf_counter() - t0)
    return out, ts


def _prune_env(value):
    if value is None:
        os.environ.pop("SRML_CAGRA_PRUNE_KERNEL", None)
    else:
        os.environ["SRML_CAGRA_PRUNE_KERNEL"] = value


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
    ap.add_argument("--graph_degree", type=int, default=32, help="of the default build")
    ap.add_argument("--configs", default="64:32,96:48",
                    help="optimised builds, intermediate_graph_degree:graph_degree")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip_ivf_pq", action="store_true")
    ap.add_argument("--skip_torch_prune", action="store_true")
    ap.add_argument("--ivf_pq_only", action="store_true",
                    help="the ivf_pq build and its search alone")
    ap.add_argument("--prune_only", action="store_true",
                    help="one nn-descent graph per config, then the kernel alone (profiler run)")
    ap.add_argument("--rehearse", action="store_true",
                    help="run without the kernels (no GPU): checks the script, times nothing real")
    args = ap.parse_args()
    configs = [tuple(int(v) for v in c.split(":")) for c in args.configs.split(",")]

    init_comm()
    dev = get_comm().device
    X, _ = gen_data.gen_blobs(args.num_rows, args.num_cols, seed=0)
    n = X.shape[0]
    nq = min(args.num_queries, n)
    itopk, width, max_it = knn_mod._cagra_search_params({}, args.k)
    report = {"num_rows": n, "num_cols": args.num_cols, "k": args.k, "num_queries": nq,
              "itopk_size": itopk, "search_width": width, "max_iterations": max_it,
              "repeats": args.repeats}
    Xt = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).to(dev)
    Qt = Xt[:nq].contiguous()
    _prune_env(None)
    on_kernel = knn_mod._cagra_prune_kernel_wanted(torch.zeros((2, 2), dtype=torch.int64, device=dev))
    report["prune_kernel_path"] = bool(on_kernel)
    if not on_kernel and not args.rehearse:
        raise SystemExit("the cagra_prune kernel is not available here: nothing to time")

    graphs = {}
    if not args.prune_only and not args.ivf_pq_only:
        base_params = {"graph_degree": args.graph_degree}
        index, ts = _timed(lambda: knn_mod._cagra_build(Xt, base_params), args.repeats,
                           "default build")
        report["build_sec[default]"] = _stats(ts)
        graphs["default"] = index.G

    for inter, degree in ([] if args.ivf_pq_only else configs):
        tag = f"{inter}->{degree}"
        if args.prune_only:
            G = knn_mod._cagra_knn_graph(Xt, inter, "nn_descent", 3)
            _timed(lambda: knn_mod._cagra_prune(G, degree), args.repeats, f"prune {tag}")
            continue
        G, ts = _timed(lambda: knn_mod._cagra_knn_graph(Xt, inter, "nn_descent", 3), args.repeats,
                       f"knn graph {tag}")
        report[f"knn_graph_sec[{tag}]"] = _stats(ts)
        (P, _), ts = _timed(lambda: knn_mod._cagra_prune(G, degree), args.repeats, f"prune {tag}")
        report[f"prune_sec[{tag}]"] = _stats(ts)
        report[f"prune_gather_GBps[{tag}]"] = round(n * inter * 4 * inter / np.median(ts) / 1e9, 1)
        if not args.skip_torch_prune:
            _prune_env("0")
            (P_t, _), ts = _timed(lambda: knn_mod._cagra_prune(G, degree), args.repeats,
                                    f"torch prune {tag}")
            _prune_env(None)
            report[f"prune_torch_sec[{tag}]"] = _stats(ts)
            report[f"prune_torch_equals_kernel[{tag}]"] = bool(torch.equal(P, P_t))
        F, ts = _timed(lambda: knn_mod._cagra_merge_reverse(P), args.repeats, f"merge {tag}")
        report[f"merge_reverse_sec[{tag}]"] = _stats(ts)
        params = {"graph_degree": degree, "intermediate_graph_degree": inter}
        index, ts = _timed(lambda: knn_mod._cagra_build(Xt, params), args.repeats, f"build {tag}")
        report[f"build_sec[{tag}]"] = _stats(ts)
        graphs[tag] = index.G
        del G, P, F

    if not args.prune_only and not args.skip_ivf_pq:
        inter, degree = configs[0]
        params = {"graph_degree": degree, "intermediate_graph_degree": inter,
                  "build_algo": "ivf_pq"}
        index, ts = _timed(lambda: knn_mod._cagra_build(Xt, params), args.repeats, "ivf_pq build")
        report[f"build_sec[ivf_pq {inter}->{degree}]"] = _stats(ts)
        graphs[f"ivf_pq {inter}->{degree}"] = index.G

    if graphs:
        df = DataFrame.from_numpy(X)
        exact = NearestNeighbors(k=args.k).fit(df)
        _, _, res = exact.kneighbors(df.take_local(np.arange(nq)))
        truth = np.asarray(res["indices"])
    for tag, G in graphs.items():
        index = knn_mod.CagraIndex(Xt=Xt, G=G)
        report[f"search_graph_width[{tag}]"] = int(G.shape[1])
        query = lambda: knn_mod._cagra_query(index, Qt, args.k, itopk, width, max_it)  # noqa: E731
        (_, ids), ts = _timed(query, args.repeats, f"search {tag}")
        report[f"search_sec[{tag}]"] = _stats(ts)
        report[f"recall@{args.k}[{tag}]"] = round(_recall(ids.cpu().numpy(), truth), 4)
        if knn_mod._cagra_kernel_wanted(index, Qt, args.k, itopk, width):
            _, _, st = knn_mod._cagra_search_kernel(index, Qt, args.k, itopk, width, max_it)
            report[f"rows_keyed_per_query[{tag}]"] = round(float(st[:, 1].double().mean()), 1)

    print(json.dumps(report))


if __name__ == "__main__":
    main()
