"""Timing of the delta KMeans step (`_accumulate_delta`) against the full pass.

Usage (on a GPU box):  python tools/time_kmeans_delta.py [--quick]

One process, bench.py's data recipe at 1M x 3000, k=1000.
  1. A fit's course: Lloyd steps 0-10 from random centres through
     `kmeans_assign_reduce`, with SRML_KMEANS_DELTA unset and =0, the two runs
     alternated (twice each). Per step: share of rows whose label changed, the
     accumulation path taken, device-event time of the whole step.
  2. The sweep behind F_DELTA: labels with 0 .. 50 % of the rows reassigned at
     random; `kmeans_label_delta` + host read of the count +
     `kmeans_delta_accumulate` (sorted and direct form) +
     `kmeans_anchor_inertia` against the full pass
     (`label_accumulate_inertia`, anchor); median of 9 and max-min.
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
ap.add_argument("--quick", action="store_true", help="3 repeats, 4 steps, one run each")
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--cols", type=int, default=3000)
ap.add_argument("--k", type=int, default=1000)
args = ap.parse_args()

real = hip_ops()
dev = torch.device("cuda:0")
REPS = 3 if args.quick else 9
STEPS = 4 if args.quick else 11
calls = []


class Ext:
    """The extension, with the names of the ops called recorded."""

    def __getattr__(self, name):
        fn = getattr(real, name)

        def wrapped(*a, **kw):
            calls.append(name)
            return fn(*a, **kw)

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


def course(delta_on):
    """[(changed share, path, ms)] over STEPS Lloyd steps from C0."""
    if delta_on:
        os.environ.pop("SRML_KMEANS_DELTA", None)
    else:
        os.environ["SRML_KMEANS_DELTA"] = "0"
    km._drop_prepared()
    C, last, rows = C0, None, []
    for _ in range(STEPS):
        calls.clear()
        ms, (labels, sums, counts, _inertia) = timed(
            lambda: km.kmeans_assign_reduce(X, C, x_sq)
        )
        if "label_accumulate_inertia" in calls:
            path = "delta+full" if "kmeans_anchor_inertia" in calls else "full"
        elif "label_accumulate" in calls:
            path = "f32 fallback"
        else:
            path = "delta" if "kmeans_delta_accumulate" in calls else "none changed"
        share = float("nan") if last is None else float((labels != last).float().mean())
        last = labels.clone()
        rows.append((share, path, ms))
        ne = counts > 0
        Cn = C.clone()
        Cn[ne] = (sums[ne] / counts[ne, None]).float()
        C = Cn
    os.environ.pop("SRML_KMEANS_DELTA", None)
    return rows, C, last


print(f"== fit course, {n} x {d}, k={k} (step 0 builds the hi plane) ==", flush=True)
runs = []
for rep in range(1 if args.quick else 2):
    for on in (True, False):
        rows, C_end, L_end = course(on)
        runs.append((on, rows))
        tag = "delta" if on else "DELTA=0"
        for i, (share, path, ms) in enumerate(rows):
            print(f"run {rep} {tag:8s} step {i:2d}: changed {100 * share:7.3f} %  "
                  f"{path:12s} {ms:8.3f} ms", flush=True)

print("== F_DELTA sweep: delta path against the full pass ==", flush=True)
ext = real
L0 = L_end.clone()
R = C_end.contiguous()
_sums, cnt32, _it, Q0, dS = ext.label_accumulate_inertia(X, L0, R, anchor=True)
S, cnt, Q, E = dS.double(), cnt32.double(), Q0.clone(), torch.zeros_like(dS, dtype=torch.float64)
prev = L0.clone()
g = torch.Generator(device=dev)
g.manual_seed(7)


def delta_path(L1, sorted_form):
    ent_lab, ent_row, n_changed = ext.kmeans_label_delta(L1, prev)
    m = int(n_changed.item())
    if m:
        ext.kmeans_delta_accumulate(X, ent_lab, ent_row, n_changed, m, R, S, cnt, Q, sorted_form)
    return ext.kmeans_anchor_inertia(R, R, S, cnt, Q, E)[0].tolist()


def full_path(L1):
    return float(ext.label_accumulate_inertia(X, L1, R, anchor=True)[2].item())


for share in (0.0, 0.001, 0.01, 0.05, 0.10, 0.25, 0.50):
    m = int(round(share * n))
    L1 = L0.clone()
    if m:
        rows_ = torch.randperm(n, generator=g, device=dev)[:m]
        L1[rows_] = ((L0[rows_].long() + 1
                      + torch.randint(0, k - 1, (m,), generator=g, device=dev)) % k).int()
    t = {"sorted": [], "direct": [], "full": []}
    for _ in range(REPS + 1):  # first round is warm-up
        for name in t:
            prev.copy_(L0)
            if name == "full":
                ms, _ = timed(lambda: full_path(L1))
            else:
                ms, _ = timed(lambda: delta_path(L1, name == "sorted"))
            t[name].append(ms)
    print(f"changed {100 * share:6.2f} %: sorted {med(t['sorted'][1:])}  "
          f"direct {med(t['direct'][1:])}  full {med(t['full'][1:])}", flush=True)
