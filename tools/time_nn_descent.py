"""Time `_nn_descent` on its two paths, the torch round and the
`nn_descent_join` kernel, in ONE process, at the two shapes that use it:

  cagra  the ANN bench's default shape (100000 x 300 blobs), degree 32, 3 rounds
  umap   the UMAP shape of profiles/umap_r02_kernel_stats.csv (1M x 256 blobs),
         degree 32, 5 rounds

Usage:
  python tools/time_nn_descent.py                    # both shapes
  python tools/time_nn_descent.py --shapes umap
  python tools/time_nn_descent.py --kernel_only      # profiler run
  python tools/time_nn_descent.py --rehearse         # no GPU: checks the script
  python tools/time_nn_descent.py --permutations 5 --shapes recall
      # torch path alone on row permutations of normal 2000 x 16: the spread
      # that sets the recall margin of tests/test_nn_descent_join_gpu.py

Per shape and path: the whole `_nn_descent` call (random start and
`_reverse_edges` included), and the step alone, round by round, which is the
seconds per round reported. One warm-up, then --repeats runs, a device
synchronise inside every timed window, medians. The torch round is also split
into its gather, `gather_dists` and sort + top-k parts on the graph its last
round starts from. The kernel's `stats` gives the mean rows keyed per node in
every round, against the J * degree + R rows the torch round keys. Recall of
both graphs is taken against the exact kNN graph on a --sample row sample.
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
from spark_rapids_ml_amd.models import knn as knn_mod  # noqa: E402
from spark_rapids_ml_amd.ops.knn import knn_topk  # noqa: E402

SHAPES = {
    # name: (rows, cols, degree, rounds)
    "cagra": (100000, 300, 32, 3),
    "umap": (1000000, 256, 32, 5),
    "recall": (2000, 16, 32, 3),
}
REHEARSAL_ROWS = 3000


def _sync():
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def _timed(fn, repeats, what=""):
    """(last result, median seconds of `repeats` calls after one warm-up)."""
    print(f"timing {what} ...", file=sys.stderr, flush=True)
    out = fn()
    ts = []
    for _ in range(repeats):
        _sync()
        t0 = time.perf_counter()
        out = fn()
        _sync()
        ts.append(time.perf_counter() - t0)
    return out, float(np.median(ts))


def _path(value):
    os.environ["SRML_NND_KERNEL"] = value


def _recall(G, Xt, sample, degree):
    """Mean share of the exact `degree` nearest neighbours of the sampled rows
    that their lists hold."""
    _, idx = knn_topk(Xt[sample].contiguous(), Xt, degree + 1)
    truth = idx.cpu().numpy()
    rows = sample.cpu().numpy()
    found = G[sample].cpu().numpy()
    hits = 0
    for r, f, t in zip(rows, found, truth):
        hits += len(set(f.tolist()) & (set(t.tolist()) - {int(r)}))
    return hits / (len(rows) * degree)


def _descent(Xt, degree, rounds, kernel):
    """`_nn_descent` with one step forced, its rounds timed one by one:
    (G, seconds of each step, mean rows keyed per node of each kernel step,
    the (G, Gd, join, rev) the last round started from)."""
    n = Xt.shape[0]
    g = torch.Generator(device="cpu")
    g.manual_seed(7)
    G = torch.randint(0, n, (n, degree), generator=g).to(Xt.device)
    Gd = knn_mod._batched_dists(Xt, None, G)
    secs, keyed, last = [], [], None
    for _ in range(rounds):
        rev = knn_mod._reverse_edges(G, min(degree, 8))
        join = torch.cat([G[:, : min(degree, 8)], rev], dim=1)
        last = (G, Gd, join, rev)
        stats = torch.zeros(n, dtype=torch.int32, device=Xt.device) if kernel else None
        _sync()
        t0 = time.perf_counter()
        if kernel:
            G, Gd = knn_mod._nnd_step_kernel(Xt, G, Gd, join, rev, stats)
        else:
            G, Gd = knn_mod._nnd_step_torch(Xt, G, Gd, join, rev)
        _sync()
        secs.append(time.perf_counter() - t0)
        if kernel:
            keyed.append(round(float(stats.double().mean()), 1))
    return G, secs, keyed, last


def _torch_split(Xt, G, Gd, join, rev, repeats):
    """Seconds of the three parts of one torch round."""
    n, degree = G.shape
    rows = torch.arange(n, device=Xt.device)
    gather = lambda: torch.cat([G[join].reshape(n, -1), rev], dim=1)  # noqa: E731
    cand, t_gather = _timed(gather, repeats, "torch gather")
    cd, t_dists = _timed(lambda: knn_mod._batched_dists(Xt, rows, cand), repeats, "gather_dists")

    def select():
        cat_i = torch.cat([G, cand], dim=1)
        cat_d = torch.cat([Gd, cd], dim=1)
        cat_d = torch.where(cat_i == rows[:, None], torch.full_like(cat_d, 3.4e38), cat_d)
        return knn_mod._dedup_topk(cat_i, cat_d, degree)

    _, t_select = _timed(select, repeats, "sort + top-k")
    return {"gather": t_gather, "gather_dists": t_dists, "sort_topk": t_select}


def _permutation_recalls(Xt, degree, rounds, count):
    """Recall of the torch path on `count` row orders of the same items."""
    n = Xt.shape[0]
    _path("0")
    out = []
    for p in range(count):
        perm = torch.from_numpy(np.random.default_rng(p).permutation(n)).to(Xt.device)
        Xp = Xt[perm].contiguous()
        G = knn_mod._nn_descent(Xp, degree, rounds)
        out.append(round(_recall(G, Xp, torch.arange(n, device=Xt.device), degree), 4))
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="cagra,umap")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sample", type=int, default=10000, help="rows of the recall sample")
    ap.add_argument("--permutations", type=int, default=0,
                    help="recall of the torch path alone on this many row orders")
    ap.add_argument("--kernel_only", action="store_true",
                    help="the kernel path alone, untimed parts skipped (profiler run)")
    ap.add_argument("--rehearse", action="store_true",
                    help="run on the CPU at a small size: checks the script, times nothing real")
    args = ap.parse_args()

    dev = torch.device("cuda" if torch.cuda.is_available() and not args.rehearse else "cpu")
    report = {"device": str(dev), "repeats": args.repeats}
    for name in args.shapes.split(","):
        n, d, degree, rounds = SHAPES[name]
        if args.rehearse:
            n = min(n, REHEARSAL_ROWS)
        if name == "recall":
            X = np.random.default_rng(0).normal(size=(n, d)).astype(np.float32)
        else:
            X, _ = gen_data.gen_blobs(n, d, seed=0)
        Xt = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).to(dev)
        _path("1")
        on_kernel = knn_mod._nnd_kernel_wanted(Xt, degree)
        if not on_kernel and not args.rehearse:
            raise SystemExit("the nn_descent_join kernel is not available here: nothing to time")
        res = {"rows": n, "cols": d, "degree": degree, "rounds": rounds,
               "torch_rows_keyed_per_node": 2 * min(degree, 8) * degree + min(degree, 8)}
        if args.permutations:
            res["torch_recall_by_permutation"] = _permutation_recalls(
                Xt, degree, rounds, args.permutations)
            report[name] = res
            continue
        sample = torch.from_numpy(
            np.random.default_rng(1).choice(n, size=min(args.sample, n), replace=False)).to(dev)
        last = None
        for path, env in (("kernel", "1"), ("torch", "0")):
            if (path == "torch" and args.kernel_only) or (path == "kernel" and not on_kernel):
                continue
            _path(env)
            _, sec = _timed(lambda: knn_mod._nn_descent(Xt, degree, rounds), args.repeats,
                            f"{name} {path}")
            res[f"{path}_nn_descent_sec"] = round(sec, 5)
            # warm from the calls above; every repeat walks the same graphs
            runs = [_descent(Xt, degree, rounds, path == "kernel") for _ in range(args.repeats)]
            per_round = np.median(np.asarray([r[1] for r in runs]), axis=0)
            res[f"{path}_step_sec_by_round"] = [round(float(v), 5) for v in per_round]
            res[f"{path}_step_sec_per_round"] = round(float(per_round.mean()), 5)
            G, _, keyed, inputs = runs[-1]
            if path == "kernel":
                res["kernel_rows_keyed_per_node"] = keyed
            else:
                last = inputs
            if not args.kernel_only:
                res[f"{path}_recall"] = round(_recall(G, Xt, sample, degree), 4)
        if last is not None:
            split = _torch_split(Xt, *last, args.repeats)
            res["torch_last_round_split_sec"] = {k: round(v, 5) for k, v in split.items()}
        report[name] = res
        del Xt
    os.environ.pop("SRML_NND_KERNEL", None)
    print(json.dumps(report))


if __name__ == "__main__":
    main()
