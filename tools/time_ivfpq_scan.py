"""Time the IVF-PQ ADC scan and the index cache at the ANN bench's default
shape (benchmark_runner.py approximate_nearest_neighbors --algorithm ivfpq),
in ONE process.

Usage:
  python tools/time_ivfpq_scan.py
  python tools/time_ivfpq_scan.py --metric inner_product --repeats 3

Scan alone: the index is built once, then SRML_IVFPQ_KERNEL=0 (torch scan)
and =1 (`ivfpq_scan_topk` kernel) alternate for --repeats rounds after one
warm-up each, with a device synchronise inside the timed window. The
candidate sets of the last round are compared, and both paths' keys are
judged against a float64 ADC of the rows they name.

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
from spark_rapids_ml_amd import ApproximateNearestNeighbors  # noqa: E402
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
        os.environ.pop("SRML_IVFPQ_KERNEL", None)
    else:
        os.environ["SRML_IVFPQ_KERNEL"] = s


def _adc_f64(index, Qt, ids):
    """float64 ADC key of the rows `ids` [nq, kc] name, chunked over queries."""
    m_sub, _, ds = index.codebooks.shape
    cb = index.codebooks.double()
    out = []
    for s0 in range(0, Qt.shape[0], 256):
        i = ids[s0 : s0 + 256].clamp(min=0)
        codes = index.codes[i].long()  # [q, kc, M]
        recon = torch.stack(
            [cb[m][codes[:, :, m]] for m in range(m_sub)], dim=2
        ).reshape(i.shape[0], i.shape[1], m_sub * ds)
        approx = index.C.double()[index.labels[i]] + recon
        q = Qt[s0 : s0 + 256, None, :].double()
        if index.mode == 1:
            out.append(-(q * approx).sum(2))
        else:
            out.append(((q - approx) ** 2).sum(2))
    return torch.cat(out)


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
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip_kneighbors", action="store_true")
    ap.add_argument("--kernel_only", action="store_true",
                    help="skip the torch scan (for a profiler run)")
    ap.add_argument("--rehearse", action="store_true",
                    help="run without the kernel (no GPU): checks the script, times nothing real")
    args = ap.parse_args()

    init_comm()
    dev = get_comm().device
    X, _ = gen_data.gen_blobs(args.num_rows, args.num_cols, seed=0)
    params = {"nlist": args.nlist, "nprobe": args.nprobe}
    nq = min(args.num_queries, X.shape[0])
    report = {"metric": args.metric, "num_rows": args.num_rows, "num_cols": args.num_cols,
              "k": args.k, "nlist": args.nlist, "nprobe": args.nprobe, "num_queries": nq}

    # -- scan alone, index built once -----------------------------------------
    Xt = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).to(dev)
    _sync()
    t0 = time.perf_counter()
    index = knn_mod._ivfpq_build(Xt, params, args.metric)
    _sync()
    report["build_sec"] = round(time.perf_counter() - t0, 4)
    Qt = index.Xt[:nq].contiguous()  # normalised already for cosine
    k_cand = min(X.shape[0], max(args.k, int(args.k * 2.0)))  # default refine_ratio
    report.update({"M": index.m_sub, "n_bits": index.n_bits, "k_cand": k_cand})

    names = {"1": "kernel"} if args.kernel_only else {"0": "torch", "1": "kernel"}
    scan = {s: [] for s in names}
    out = {}
    for s in names:  # warm-up
        _set_env(s)
        report[f"kernel_path[SRML_IVFPQ_KERNEL={s}]"] = bool(
            knn_mod._ivfpq_kernel_wanted(index, Qt, k_cand)
        )
        knn_mod._ivfpq_candidates(index, Qt, args.nprobe, k_cand)
    if not report["kernel_path[SRML_IVFPQ_KERNEL=1]"] and not args.rehearse:
        raise SystemExit("the ivfpq_scan_topk kernel is not available here: nothing to time")
    for _ in range(args.repeats):
        for s in names:
            _set_env(s)
            _sync()
            t0 = time.perf_counter()
            out[s] = knn_mod._ivfpq_candidates(index, Qt, args.nprobe, k_cand)
            _sync()
            scan[s].append(time.perf_counter() - t0)
    for s, name in names.items():
        report[f"scan_only_sec[{name}]"] = _stats(scan[s])
    for s, name in names.items():
        key, ids = out[s]
        ref = _adc_f64(index, Qt, ids)
        live = ids >= 0
        report[f"max_abs_key_err_vs_f64_adc[{name}]"] = (
            (key.double() - ref)[live].abs().max().item()
        )
        report[f"median_key[{name}]"] = ref[live].median().item()
    if len(names) == 2:
        report["torch_fastest_over_kernel_median"] = (
            report["scan_only_sec[torch]"]["min"] / report["scan_only_sec[kernel]"]["median"]
        )
        ids_t, ids_k = out["0"][1], out["1"][1]
        same = (ids_t.sort(dim=1).values == ids_k.sort(dim=1).values).all(dim=1)
        report["scan_rows_with_same_candidate_set"] = f"{int(same.sum())}/{nq}"
        a, b = ids_t.cpu().numpy(), ids_k.cpu().numpy()
        inter = sum(len(set(x.tolist()) & set(y.tolist())) for x, y in zip(a, b))
        report["candidate_overlap"] = inter / a.size
    del out

    # -- whole kneighbors: first call (build + query) against second ---------
    if not args.skip_kneighbors:
        _set_env("default")
        df = DataFrame.from_numpy(X)
        q = df.take_local(np.arange(nq))
        first, second = [], []
        for r in range(args.repeats + 1):  # round 0 is the warm-up
            model = ApproximateNearestNeighbors(
                k=args.k, algorithm="ivfpq", metric=args.metric, algoParams=params,
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
