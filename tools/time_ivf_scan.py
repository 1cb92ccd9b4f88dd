"""Time ApproximateNearestNeighbors.kneighbors (ivfflat) at the ANN bench's
default shape, alternating SRML_IVF_KERNEL settings in ONE process.

Usage:
  python tools/time_ivf_scan.py --metric sqeuclidean --settings 0,1 --scan
  python tools/time_ivf_scan.py --metric euclidean --settings default,1

Each setting is warmed up once, then the settings alternate for --repeats
rounds with a device synchronise inside the timed window. With two settings
the neighbour sets of the last round are compared. --scan additionally times
the probed-list scan alone (index built once) with the torch path and the
`ivf_scan_topk` kernel, and judges the rows where they name different
neighbours against float64 distances. Prints one JSON line.
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
from spark_rapids_ml_amd import ApproximateNearestNeighbors  # noqa: E402
from spark_rapids_ml_amd.data import DataFrame  # noqa: E402
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
        os.environ.pop("SRML_IVF_KERNEL", None)
    else:
        os.environ["SRML_IVF_KERNEL"] = s


def main() -> None:
    ap = argparse.ArgumentParser()
    # defaults = benchmark_runner.py approximate_nearest_neighbors defaults
    ap.add_argument("--num_rows", type=int, default=100000)
    ap.add_argument("--num_cols", type=int, default=300)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--num_queries", type=int, default=10000)
    ap.add_argument("--nlist", type=int, default=256)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--metric", default="euclidean")
    ap.add_argument("--settings", default="default",
                    help="comma list of SRML_IVF_KERNEL values: default|0|1")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scan", action="store_true")
    args = ap.parse_args()

    init_comm()
    X, _ = gen_data.gen_blobs(args.num_rows, args.num_cols, seed=0)
    df = DataFrame.from_numpy(X)
    nq = min(args.num_queries, len(df))
    q = df.take_local(np.arange(nq))
    model = ApproximateNearestNeighbors(
        k=args.k, algorithm="ivfflat", metric=args.metric,
        algoParams={"nlist": args.nlist, "nprobe": args.nprobe},
    ).fit(df)

    settings = args.settings.split(",")
    times = {s: [] for s in settings}
    idx = {}
    for s in settings:  # warm-up
        _set_env(s)
        model.kneighbors(q)
    for _ in range(args.repeats):
        for s in settings:
            _set_env(s)
            _sync()
            t0 = time.perf_counter()
            _, _, knn_df = model.kneighbors(q)
            _sync()
            times[s].append(time.perf_counter() - t0)
            idx[s] = np.asarray(knn_df["indices"])

    report = {"metric": args.metric, "num_rows": args.num_rows, "num_cols": args.num_cols,
              "k": args.k, "nlist": args.nlist, "nprobe": args.nprobe, "num_queries": nq}
    for s in settings:
        report[f"kneighbors_sec[SRML_IVF_KERNEL={s}]"] = _stats(times[s])
    if len(settings) == 2:
        a, b = idx[settings[0]], idx[settings[1]]
        same = sum(set(x.tolist()) == set(y.tolist()) for x, y in zip(a, b))
        inter = sum(len(set(x.tolist()) & set(y.tolist())) for x, y in zip(a, b))
        report["rows_with_same_neighbour_set"] = f"{same}/{len(a)}"
        report["neighbour_overlap"] = inter / a.size

    if args.scan:
        from spark_rapids_ml_amd.models import knn as knn_mod

        dev = get_comm().device
        Xt = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).to(dev)
        Qt = Xt[:nq].contiguous()
        C, labels = model._build_coarse(Xt, args.nlist)
        scan = {False: [], True: []}
        out = {}

        def run(uk):
            return knn_mod._ivf_search(
                Qt, Xt, C, labels, args.nlist, args.nprobe, args.k, 0, use_kernel=uk
            )

        for uk in (False, True):
            run(uk)
        for _ in range(args.repeats):
            for uk in (False, True):
                _sync()
                t0 = time.perf_counter()
                out[uk] = run(uk)
                _sync()
                scan[uk].append(time.perf_counter() - t0)
        report["scan_only_sec[torch]"] = _stats(scan[False])
        report["scan_only_sec[kernel]"] = _stats(scan[True])

        # float64 distances of the rows each path names
        def true_d(ids):
            parts = []
            for s0 in range(0, nq, 500):
                i = ids[s0 : s0 + 500].clamp(min=0)
                parts.append(((Qt[s0 : s0 + 500, None, :].double() - Xt[i].double()) ** 2).sum(2))
            return torch.cat(parts)

        (key_t, ids_t), (key_k, ids_k) = out[False], out[True]
        dt, dk = true_d(ids_t), true_d(ids_k)
        report["max_abs_key_err_vs_f64[torch]"] = (key_t.double() - dt).abs().max().item()
        report["max_abs_key_err_vs_f64[kernel]"] = (key_k.double() - dk).abs().max().item()
        report["median_key"] = dt.median().item()
        same = (ids_t.sort(dim=1).values == ids_k.sort(dim=1).values).all(dim=1)
        report["scan_rows_differ"] = int((~same).sum())
        # smaller sum of true distances = the better neighbour set
        st, sk = dt.sum(1)[~same], dk.sum(1)[~same]
        report["differing_rows_kernel_set_at_least_as_good"] = int((sk <= st).sum())
        gap = (dt.sort(dim=1).values - dk.sort(dim=1).values).abs() / dt.sort(dim=1).values.clamp(min=1e-30)
        report["max_rel_gap_between_named_neighbours"] = gap.max().item()

    print(json.dumps(report))


if __name__ == "__main__":
    main()
