"""A/B timing of the KMeans assignment: f32 GEMM path vs split-bf16 screen.

Usage (on a GPU box):  python tools/time_assign_split.py [--quick]

One process, bench.py's data recipe at 1M x 3000, k=1000. Alternates
`_assign_gemm(layout="kn")` and `_assign_split`, 9 repeats each after
warm-up, device-event timed; prints median and max-min per side and the
flagged fraction. Run with random centres and with centres after 3 Lloyd
steps. Then the two sweeps behind ops/kmeans.py's D_MIN and F_MAX:
  - columns d at k=1000 (randn data)
  - flagged fraction, raised by duplicating a share of the centres pairwise
    (every row nearest a duplicated pair is flagged with two candidates).
    Blending all centres towards one row does not raise it: after centring
    that only scales c', and the margin scales with it (one line shows this).

--prepared times the prepared-X step instead (`_assign_prepared`): the whole
`kmeans_assign_reduce` with SRML_KMEANS_CACHE on and off over the first Lloyd
steps (flagged share per step), then each part of the hi path and of a
fall-up on the centres after those steps: the costs behind F_HI.
"""
import argparse
import sys

import torch

sys.path.insert(0, ".")
import spark_rapids_ml_amd.ops.kmeans as km
from spark_rapids_ml_amd.ops.dispatch import hip_ops

ap = argparse.ArgumentParser()
ap.add_argument("--quick", action="store_true", help="3 repeats, short sweeps")
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--prepared", action="store_true", help="time the prepared-X step only")
args = ap.parse_args()

real = hip_ops()
dev = torch.device("cuda:0")
REPS = 3 if args.quick else 9
flag_counts = []


class Ext:
    """The extension, with the screen's flagged count recorded."""

    def __getattr__(self, name):
        return getattr(real, name)

    @staticmethod
    def kmeans_argmin_kn_screen(*a):
        out = real.kmeans_argmin_kn_screen(*a)
        flag_counts.append(out[4])
        return out


ext = Ext()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def ab(X, C, x_sq, reps=REPS):
    n, k = X.shape[0], C.shape[0]
    f32 = lambda: km._assign_gemm(ext, X, C, x_sq, n, k, layout="kn")  # noqa: E731
    split = lambda: km._assign_split(ext, X, C, x_sq, n, k)  # noqa: E731
    f32(), split()
    torch.cuda.synchronize()
    flag_counts.clear()
    tf, ts = [], []
    for _ in range(reps):
        tf.append(timed(f32))
        ts.append(timed(split))
    flagged = sum(int(c.item()) for c in flag_counts) / max(1, reps)
    tf.sort(), ts.sort()
    return (tf[len(tf) // 2], tf[-1] - tf[0], ts[len(ts) // 2], ts[-1] - ts[0], flagged / n)


def show(tag, r):
    print(f"{tag}: f32 {r[0]:.2f} ms ({r[1]:.2f})  split {r[2]:.2f} ms ({r[3]:.2f})  "
          f"ratio {r[0] / r[2]:.2f}x  flagged {100 * r[4]:.3f} %", flush=True)


n, d, k = args.rows, 3000, 1000
gen = torch.Generator(device=dev)
gen.manual_seed(1234)
latent = torch.randn(k, d, generator=gen, device=dev)
X = torch.empty(n, d, device=dev)
for s in range(0, n, 1 << 18):
    e = min(n, s + (1 << 18))
    assign = torch.randint(0, k, (e - s,), generator=gen, device=dev)
    X[s:e] = latent[assign] + 0.5 * torch.randn(e - s, d, generator=gen, device=dev)
x_sq = (X * X).sum(dim=1)
g0 = torch.Generator(device=dev)
g0.manual_seed(42)
C0 = torch.randn(k, d, generator=g0, device=dev)



def med(fn, reps=REPS):
    fn()
    torch.cuda.synchronize()
    ts = sorted(timed(fn) for _ in range(reps))
    return ts[len(ts) // 2], ts[-1] - ts[0]


def prepared_report():
    import os

    km.hip_ops = lambda: ext

    def lloyd(C, steps, tag):
        for i in range(steps):
            flag_counts.clear()
            t = timed(lambda: km.kmeans_assign_reduce(X, C, x_sq))
            fl = [int(c.item()) for c in flag_counts]
            labels, sums, counts, inertia = km.kmeans_assign_reduce(X, C, x_sq)
            print(f"  {tag} step {i}: {t:.2f} ms  flagged per screen {fl}  "
                  f"inertia {inertia!r}", flush=True)
            nz = counts > 0
            Cn = C.clone()
            Cn[nz] = (sums[nz] / counts[nz, None]).float()
            C = Cn
        return C

    os.environ["SRML_KMEANS_CACHE"] = "0"
    lloyd(C0, 6, "cache off")
    del os.environ["SRML_KMEANS_CACHE"]
    C = lloyd(C0, 6, "cache on ")

    for tag, env in (("cache off", "0"), ("cache on ", "1")):
        os.environ["SRML_KMEANS_CACHE"] = env
        t, sp = med(lambda: km.kmeans_assign_reduce(X, C, x_sq))
        print(f"step on converged C, {tag}: {t:.2f} ms ({sp:.2f})", flush=True)
    del os.environ["SRML_KMEANS_CACHE"]

    prep = km._prepared(real, X, C)
    SC, c_sq = real.kmeans_split_bf16(C, prep.mu)
    dp = SC.shape[1] // 2
    Ch = SC[:, :dp].contiguous()
    ClCh = torch.cat([SC[:, dp:], SC[:, :dp]], dim=1)
    dots = torch.empty((k, n), dtype=torch.float32, device=dev)
    margin = ((4.0 * km.EPS_HI) * c_sq.max().sqrt()).reshape(1)
    gb = dots.numel() * 4 / 1e9

    def line(tag, r, extra=""):
        print(f"  {tag:34s} {r[0]:7.2f} ms ({r[1]:.2f}) {extra}", flush=True)

    line("hi split of X (once per fit)", med(lambda: real.kmeans_split_bf16_hi(X, prep.mu)))
    r = med(lambda: torch.mm(Ch, prep.H.T, out_dtype=torch.float32, out=dots))
    line("K=dp GEMM", r, f"{2.0 * n * k * dp / r[0] / 1e9:.0f} TF")
    r = med(lambda: real.kmeans_argmin_kn_screen(dots, prep.a_sq, c_sq, margin))
    line("kmeans_argmin_kn_screen", r, f"{gb / r[0]:.2f} TB/s")
    r = med(lambda: real.kmeans_argmin_kn(dots, prep.a_sq, c_sq))
    line("kmeans_argmin_kn, same block", r, f"{gb / r[0]:.2f} TB/s")
    labels = real.kmeans_argmin_kn_screen(dots, prep.a_sq, c_sq, margin)[0]
    line("label_accumulate", med(lambda: real.label_accumulate(X, labels, k)))
    line("label_accumulate_inertia vec", med(lambda: real.label_accumulate_inertia(X, labels, C, True)))
    line("label_accumulate_inertia scalar", med(lambda: real.label_accumulate_inertia(X, labels, C, False)))
    SX = real.kmeans_split_bf16(X, prep.mu)[0]
    line("fall-up: kmeans_split_bf16 of X", med(lambda: real.kmeans_split_bf16(X, prep.mu)))
    line("fall-up: addmm K=2dp", med(
        lambda: torch.addmm(dots, ClCh, SX.T, out_dtype=torch.float32, out=dots)))
    del SX
    for share in (0.01, 0.05, 0.10, 0.25):
        rows = torch.randperm(n, device=dev)[: int(share * n)].sort().values
        r = med(lambda: km._refine_f32(real, X, C, x_sq, rows), reps=3)
        line(f"_refine_f32 on {100 * share:.0f} % of the rows", r,
             f"{r[0] * 1e6 / rows.numel():.1f} ns/row")


if args.prepared:
    prepared_report()
    sys.exit(0)

# the screen must never fall back while it is being timed
f_max = km.F_MAX
km.F_MAX = 2.0

show(f"{n}x{d} k={k}, random C", ab(X, C0, x_sq))
C = C0
for _ in range(3):
    labels, sums, counts, _inertia = km.kmeans_assign_reduce(X, C, x_sq)
    nz = counts > 0
    Cn = C.clone()
    Cn[nz] = (sums[nz] / counts[nz, None]).float()
    C = Cn
show(f"{n}x{d} k={k}, C after 3 Lloyd steps", ab(X, C, x_sq))

print("flagged-fraction sweep (share of centres duplicated pairwise):")
for share in ([0.1, 0.5] if args.quick else [0.02, 0.05, 0.1, 0.2, 0.4, 0.7, 1.0]):
    Cd = C.clone()
    m = int(share * k) // 2 * 2
    Cd[1:m:2] = Cd[0:m:2]
    show(f"  duplicated {share:.2f}", ab(X, Cd, x_sq, reps=3))
Cb = 0.001 * C + 0.999 * C[:1]
show("  blended 0.999 towards C[0]", ab(X, Cb, x_sq, reps=3))
del X, x_sq

print("d sweep at k=1000 (randn):")
for dd in ([64, 512] if args.quick else [32, 64, 128, 256, 512, 1024]):
    Xd = torch.randn(n, dd, generator=gen, device=dev)
    Cd = torch.randn(k, dd, generator=gen, device=dev)
    show(f"  d={dd}", ab(Xd, Cd, (Xd * Xd).sum(1), reps=5))
    del Xd
km.F_MAX = f_max
