"""Time the RandomForest paths that rf_best_split_scan and fil_predict_wide
serve against the torch paths they replace, alternating the two in ONE process.

Usage:
  python tools/time_rf_wide.py                      # every section below
  python tools/time_rf_wide.py --sections fit --classes 32 --repeats 1

Data: `--rows` x `--cols` standard-normal features (the RFC benchmark shape by
default), labels re-drawn as the argmax of C random linear scores. Sections:

- `fit`: classification fit with C in --classes, default scan against
  SRML_RF_SCAN=torch (the torch cumsum/max scan over the kernel histogram).
  Each setting is fitted once untimed, then per repeat once with the timers
  off (fit wall, ends in a device synchronise) and once with SRML_RF_DEBUG=2
  (the grow loop's `hist_scan` seconds). The two models are compared.
- `entropy`: 2-class fit, impurity gini (rf_best_split) against entropy
  (rf_best_split_scan), same two numbers.
- `transform`: forest_predict (fil_predict_wide) against forest_traverse on the
  device-resident rows with each C-class forest, and the largest difference.

Prints one JSON line per measurement.
"""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from spark_rapids_ml_amd import RandomForestClassifier  # noqa: E402
from spark_rapids_ml_amd.data import DataFrame  # noqa: E402
from spark_rapids_ml_amd.ops import forest  # noqa: E402

_last_acc = {}
_report = forest.RFTimer.report


def _keep_report(self):
    _last_acc.update(self.acc)
    _report(self)


forest.RFTimer.report = _keep_report


def _stats(ts):
    a = np.asarray(ts)
    return {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max())}


def _fit(df, args, impurity, scan, debug):
    for key, val in (("SRML_RF_SCAN", scan), ("SRML_RF_DEBUG", debug)):
        if val is None:
            os.environ.pop(key, None)
        else:
            os.environ[key] = val
    _last_acc.clear()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model = RandomForestClassifier(
        numTrees=args.trees, maxDepth=args.depth, maxBins=args.bins, seed=1, impurity=impurity
    ).fit(df)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, _last_acc.get("hist_scan"), model


def _same_trees(a, b):
    """How far two forests agree. A tree's nodes are numbered level by level,
    so the nodes before its first differing split were chosen from the same
    rows: the largest gain difference among them, the shallowest depth at
    which any tree differs, and the gain difference of the splits that differ
    AT that depth (a near-tie that f32 and f64 arithmetic order differently
    shows as a tiny one). All trees grow in one arena and share the feature
    sampler, so below that depth the forests draw other feature subsets and
    are no longer comparable node by node."""
    gap, firsts = 0.0, []
    for ta, tb in zip(a.trees, b.trees):
        m = min(ta["feature"].shape[0], tb["feature"].shape[0])
        eq = (ta["feature"][:m] == tb["feature"][:m]) & (ta["threshold"][:m] == tb["threshold"][:m])
        first = m if eq.all() else int(np.argmin(eq))
        if first:
            gap = max(gap, float(np.abs(ta["gain"][:first] - tb["gain"][:first]).max()))
        if first < m:
            depth = np.zeros(first + 1, np.int64)
            for i in range(first + 1):  # parents precede children
                for c in (ta["left"][i], ta["right"][i]):
                    if 0 <= c <= first and i < first:
                        depth[c] = depth[i] + 1
            firsts.append((int(depth[first]), float(abs(ta["gain"][first] - tb["gain"][first]))))
    if not firsts:
        return {"trees_identical": True, "max_gain_gap": gap}
    d0 = min(d for d, _ in firsts)
    return {"trees_identical": False, "max_gain_gap_before_difference": gap,
            "first_difference_depth": d0,
            "max_gain_gap_at_first_difference": max(g for d, g in firsts if d == d0)}


def _ab_fit(name, df, args, settings):
    """settings: two (label, impurity, scan) triples, alternated."""
    wall = {s[0]: [] for s in settings}
    scan_s = {s[0]: [] for s in settings}
    models = {}
    for label, impurity, scan in settings:  # warm-up
        _fit(df, args, impurity, scan, None)
    for _ in range(args.repeats):
        for label, impurity, scan in settings:
            w, _, models[label] = _fit(df, args, impurity, scan, None)
            wall[label].append(w)
            _, h, _ = _fit(df, args, impurity, scan, "2")
            scan_s[label].append(h)
    out = {"case": name}
    for label, _, _ in settings:
        out[label] = {"fit_wall_sec": _stats(wall[label]), "hist_scan_sec": _stats(scan_s[label])}
    if settings[0][1] == settings[1][1]:
        out.update(_same_trees(models[settings[0][0]], models[settings[1][0]]))
    print(json.dumps(out), flush=True)
    return models[settings[0][0]]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sections", default="fit,entropy,transform")
    ap.add_argument("--classes", default="32,100")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--cols", type=int, default=3000)
    ap.add_argument("--trees", type=int, default=10)
    ap.add_argument("--depth", type=int, default=13)
    ap.add_argument("--bins", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_rf_wide.py measures on the GPU"
    sections = args.sections.split(",")
    gen = torch.Generator(device="cuda").manual_seed(0)
    Xt = torch.randn(args.rows, args.cols, generator=gen, device="cuda")
    X = Xt.cpu().numpy()
    shape = f"{args.rows}x{args.cols} {args.trees} trees d{args.depth} b{args.bins}"

    def frame(C):
        W = torch.randn(args.cols, C, generator=gen, device="cuda")
        return DataFrame.from_numpy(X, (Xt @ W).argmax(dim=1).cpu().numpy().astype(np.float64))

    for C in [int(v) for v in args.classes.split(",")]:
        df = frame(C)
        if "fit" in sections:
            model = _ab_fit(f"fit C={C} {shape}", df, args,
                            [("kernel", "gini", None), ("torch", "gini", "torch")])
        else:
            model = _fit(df, args, "gini", None, None)[2]
        if "transform" in sections:
            arena = model._device_arena
            calls = {
                "kernel": lambda: forest.forest_predict(Xt, model.trees, "classification", C, arena),
                "torch": lambda: forest.forest_traverse(Xt, model.trees, "classification", C),
            }
            times = {k: [] for k in calls}
            outs = {k: fn() for k, fn in calls.items()}  # warm-up
            for _ in range(args.repeats):
                for k, fn in calls.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    outs[k] = fn()
                    torch.cuda.synchronize()
                    times[k].append(time.perf_counter() - t0)
            print(json.dumps({
                "case": f"transform C={C} {args.rows} rows, {args.trees} trees",
                "kernel_sec": _stats(times["kernel"]), "torch_sec": _stats(times["torch"]),
                "max_abs_diff": float((outs["kernel"] - outs["torch"]).abs().max()),
            }), flush=True)
    if "entropy" in sections:
        _ab_fit(f"fit C=2 {shape}", frame(2), args,
                [("gini", "gini", None), ("entropy", "entropy", None)])


if __name__ == "__main__":
    main()
