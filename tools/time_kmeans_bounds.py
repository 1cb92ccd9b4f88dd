"""Timing of the row-bounds KMeans step (`_assign_bounded`) against the full screen.

Usage (on a GPU box):  python tools/time_kmeans_bounds.py [--quick]

One process, bench.py's data recipe at 1M x 3000, k=1000.
  1. A fit's course: Lloyd steps 0-10 from random centres through
     `kmeans_assign_reduce`, with SRML_KMEANS_BOUNDS unset and =0, the two runs
     alternated (twice each). Per step: rows the bound test left active, the
     assignment path taken, device-event time of the whole step.
  2. The sweep behind F_SKIP: the reference state of the converged fit with
     the gap of 0 .. 50 % of the rows, chosen at random, set to 0 (on top of
     its own near-ties), so that many rows are active at zero drift;
     `_assign_prepared` with the bound path forced against the same call with
     SRML_KMEANS_BOUNDS=0; median of 9 and max-min.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, ".")
import spark_rapids_ml_amd.ops.kmeans as km
from spark_rapids_ml_amd.ops.dispatch import hip_ops

ap = argparse.ArgumentParser()
ap.add_argument("--quick", action="store_true", help="3 repeats, 5 steps, one run each")
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--cols", type=int, default=3000)
ap.add_argument("--k", type=int, default=1000)
args = ap.parse_args()

real = hip_ops()
dev = torch.device("cuda:0")
REPS = 3 if args.quick else 9
STEPS = 5 if args.quick else 11
calls = []
active = []


class Ext:
    """The extension, with the names of the ops called recorded, and the
    count `kmeans_bound_test` returned."""

    def __getattr__(self, name):
        fn = getattr(real, name)

        def wrapped(*a, **kw):
            calls.append(name)
            out = fn(*a, **kw)
            if name == "kmeans_bound_test":
                active.append(out[1])
            return out

        return wrapped


km.hip_ops = lambda: Ext()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def med(ts):
    return f"{statistics.median(ts):7.3f} ms (spread {max(ts) - min(ts):.3f})"


n, d, k = args.rows, args.cols, args.k
gen = torch.Generator(device=dev)
gen.manual_seed(1234)
latent = torch.randn(k, d, generator=gen, device=dev)
X = torch.empty(n, d, device=dev)
for s in range(0, n, 1 << 18):
    e = min(n, s + (1 << 18))
    assign = torch.randint(0, k, (e - s,), generator=gen, device=dev)
    X[s:e] = latent[assign] + 0.5 * torch.randn(e - s, d, generator=gen, device=dev)
x_sq = (X * X).sum(1)
g0 = torch.Generator(device=dev)
g0.manual_seed(42)
C0 = torch.randn(k, d, generator=g0, device=dev)


def course(bounds_on):
    """[(active rows or None, path, ms)] over STEPS Lloyd steps from C0."""
    if bounds_on:
        os.environ.pop("SRML_KMEANS_BOUNDS", None)
    else:
        os.environ["SRML_KMEANS_BOUNDS"] = "0"
    km._drop_prepared()
    C, rows, Cs = C0, [], []
    for _ in range(STEPS):
        calls.clear()
        active.clear()
        Cs.append(C)
        ms, (_labels, sums, counts, _inertia) = timed(
            lambda: km.kmeans_assign_reduce(X, C, x_sq)
        )
        m = int(active[0].item()) if active else None
        if "kmeans_bound_test" not in calls:
            path = "reference"
        elif calls.count("kmeans_argmin_kn_screen") and "kmeans_gather_rows_bf16" not in calls:
            path = "test+reference"
        else:
            path = "bounds"
        rows.append((m, path, ms))
        ne = counts > 0
        Cn = C.clone()
        Cn[ne] = (sums[ne] / counts[ne, None]).float()
        C = Cn
    os.environ.pop("SRML_KMEANS_BOUNDS", None)
    return rows, Cs


print(f"== fit course, {n} x {d}, k={k} (step 0 builds the hi plane) ==", flush=True)
for rep in range(1 if args.quick else 2):
    for on in (True, False):
        rows, Cs = course(on)
        tag = "bounds" if on else "BOUNDS=0"
        for i, (m, path, ms) in enumerate(rows):
            act = "      -" if m is None else f"{m:7d}"
            print(f"run {rep} {tag:8s} step {i:2d}: active {act}  {path:14s} {ms:8.3f} ms",
                  flush=True)

print("== F_SKIP sweep: bound path at zero drift against the full screen ==", flush=True)
km.hip_ops = lambda: real
C = Cs[-1]
km._drop_prepared()
km.kmeans_assign_reduce(X, C, x_sq)  # reference pass at C
prep = km._PREP
assert prep is not None and prep.ref_k == k
gap0 = prep.gap_ref.clone()
print(f"near-ties of the reference pass: {int((gap0 == 0).sum())} rows", flush=True)
g = torch.Generator(device=dev)
g.manual_seed(7)
km.F_SKIP = 1.0  # the sweep decides where it belongs


def assign(bounds_on):
    if bounds_on:
        os.environ.pop("SRML_KMEANS_BOUNDS", None)
    else:
        os.environ["SRML_KMEANS_BOUNDS"] = "0"
    return km._assign_prepared(real, X, C, x_sq, prep)[0]


for share in (0.0, 0.001, 0.01, 0.05, 0.10, 0.25, 0.50):
    m = int(round(share * n))
    gap = gap0.clone()
    if m:
        gap[torch.randperm(n, generator=g, device=dev)[:m]] = 0.0
    t = {"bounds": [], "full": []}
    for _ in range(REPS + 1):  # first round is warm-up
        for name in t:
            # the BOUNDS=0 call marks the state stale: put it back; no label
            # changed, so the F_TRY gate is open
            prep.gap_ref, prep.ref_k, prep.changed = gap, k, 0
            ms, _ = timed(lambda: assign(name == "bounds"))
            t[name].append(ms)
    print(f"active {100 * share:6.2f} % + near-ties: bounds {med(t['bounds'][1:])}  "
          f"full {med(t['full'][1:])}", flush=True)
os.environ.pop("SRML_KMEANS_BOUNDS", None)
