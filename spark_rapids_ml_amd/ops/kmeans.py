"""KMeans ops: assignment (distance + argmin) + accumulation.

HIP path (gfx950), large k and d >= D_MIN: `kmeans_split_bf16` centres and
splits X and C into bf16 hi|lo halves, the library bf16 GEMM (f32 out) screens
every (row, centre) pair at the bf16 MFMA rate, `kmeans_argmin_kn_screen`
decides the rows it can, and the near-ties are decided as the f32 path
decides them (`_refine_f32`) or, on request, in f64 by `kmeans_refine`
(`_assign_split`). Otherwise the f32 library GEMM + `kmeans_argmin_kn` /
`kmeans_argmin_nk` epilogues (`_assign_gemm`), or `kmeans_assign` — LDS-tiled
‖x‖²+‖c‖²−2x·c on mfma_f32_32x32x2f32 with a fused per-row argmin.
`label_accumulate` is the vectorized per-center sum/count scatter.

Small k (k < 384) with centres that fit in LDS: `kmeans_assign_reduce` runs the
whole step in `kmeans_step_resident` (`_resident_wanted`) — one pass over X,
the centres resident in LDS, dots and the one-hot sum accumulation both on
mfma_f32_32x32x2f32, no [n, k] dot block in global memory, block partials
reduced in f64 (bit-reproducible for a fixed grid). It is the default there
(159 against 164 ms per step at 100M×128, k=200; 0.28 against 0.53 ms at
1M×32, k=16; RESULTS.md); SRML_KMEANS_VARIANT=f32 keeps the GEMM +
`kmeans_argmin_nk` + `label_accumulate` path, =resident asks for the kernel
wherever it is legal. `kmeans_predict` does not use it.

Across the calls of one fit X does not change, so `kmeans_assign_reduce`
keeps the centred bf16 hi plane of X and |x'|² (`_prepared`, one entry,
SRML_KMEANS_CACHE=0 disables it) and screens with the hi·hi term alone
(`_assign_prepared`): one K=dp GEMM instead of three terms and no split pass
over X. A chunk with too many near-ties adds the other two terms onto the
same dot block. That path reports the inertia `label_accumulate_inertia`
sums beside the accumulation, as (x − c)² directly.

The same cache entry carries the accumulation from step to step
(`_accumulate_delta`, SRML_KMEANS_DELTA=0 disables it): a private copy of the
last labels and, per centre, the count, Σ(x − r) and Σ|x − r|² about an anchor
r, the centre at the last full pass. `kmeans_label_delta` lists the rows whose
label changed, `kmeans_delta_accumulate` moves them between their centres'
moments (X is read at those rows only) and `kmeans_anchor_inertia` evaluates
sums and inertia for the current centres; 7.1 against 9.9 ms per step once few
rows change (profiles/README.md "Delta step"). The full pass over X runs on a
fresh entry or another k, when more than `F_DELTA` of the rows changed, and
when the centres have drifted from their anchors by more than the rows lie
around them.

It also carries the assignment (`_assign_bounded`, SRML_KMEANS_BOUNDS=0
disables it): the centres, labels and certified per-row gaps of the last pass
that screened every row. `kmeans_centre_drift` and `kmeans_bound_test` keep
the label of every row whose gap exceeds what the centres' drift since can
have changed; the others are gathered (`kmeans_gather_rows_bf16`) and take the
GEMM and the screen on their own; 2.8 against 7.1 ms per step
(profiles/README.md "Row bounds").

f64 rows (float32_inputs=False) have a path of their own, `_step_f64`:
`kmeans_assign_f64` forms c² − 2x·c on mfma_f64_16x16x4f64 with the running
(score, index) argmin in registers (lower index on an exact tie) and per-block
inertia partials, and `label_accumulate_f64` sums the sorted segments in
doubles into per-split partials reduced in a fixed order. Neither uses a
floating atomic, so a step is bitwise repeatable; any n, k, d is legal.
SRML_KMEANS_VARIANT, the prepared-X cache and the resident kernel are f32-only
and are not consulted. `kmeans_predict` takes the same assign kernel.

Together these are the KMeansMG Lloyd-step kernel family of the reference
(clustering.py:381-415).
"""

from __future__ import annotations

import os
import weakref
from typing import Optional, Tuple

import torch

from . import torch_ref
from .dispatch import hip_ops, use_hip


def kmeans_assign_reduce(
    X: torch.Tensor,
    C: torch.Tensor,
    x_sq: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, float]:
    """Returns (labels i32 [n], sums [k,d], counts [k], inertia).

    Default GPU path at the 1M×3000×k=1000 headline shape: the split-bf16
    screen (`_assign_split`, 22.7 ms against 43.8 ms for the f32 GEMM path,
    profiles/README.md) + `label_accumulate`. SRML_KMEANS_VARIANT=f32 keeps
    the hipBLASLt f32 GEMM (141 TF) + `kmeans_argmin_kn` epilogue, =fused the
    all-in-one MFMA `kmeans_assign` kernel (84 TF), =split forces the screen
    below D_MIN columns, =split_f64 also decides its near-ties in f64.

    Where the dispatch takes the screen and X is a contiguous device tensor,
    the hi plane of X is prepared once and reused while the same X comes back
    (`_prepared`; 9.8 against 27.4 ms per step, profiles/README.md). The
    cache recognises X by identity, storage address, shape and torch's
    version counter: a write to X that bypasses that counter (through
    `.data`, a raw pointer, another library) is not seen.
    SRML_KMEANS_CACHE=0 turns the cache off.

    At k < 384 a contiguous f32 device X whose centres fit in LDS takes the
    one-pass `kmeans_step_resident` kernel (`_resident_wanted`).

    An f64 device X (float32_inputs=False) takes `_step_f64`: everything
    above is f32-only and is not consulted for it."""
    if use_hip(X) and X.dtype == torch.float64:
        return _step_f64(hip_ops(), X, C, x_sq)
    if use_hip(X) and X.dtype == torch.float32:
        ext = hip_ops()
        if x_sq is None:
            x_sq = _xsq(X)
        if _cache_applies(X, C):
            prep = _prepared(ext, X, C)
            if prep is not None:
                variant = os.environ.get("SRML_KMEANS_VARIANT")
                labels, inertia = _assign_prepared(
                    ext, X, C, x_sq, prep, exact=variant == "split_f64"
                )
                if inertia is None:
                    if os.environ.get("SRML_KMEANS_DELTA") != "0":
                        return (labels, *_accumulate_delta(ext, X, labels, C, prep))
                    prep.k = 0  # the moments miss this step: not to be resumed
                    sums, counts, inertia = ext.label_accumulate_inertia(
                        X, labels, C.contiguous()
                    )
                else:  # ended in `_fallback_f32`
                    sums, counts = ext.label_accumulate(X, labels, C.shape[0])
                return (labels, sums.to(torch.float64), counts.to(torch.float64),
                        float(inertia.item()))
        if _resident_wanted(X, C):
            return _step_resident(ext, X, C, x_sq)
        X = X.contiguous()
        labels, inertia = _assign(ext, X, C, x_sq)
        sums, counts = ext.label_accumulate(X, labels, C.shape[0])
        return labels, sums.to(torch.float64), counts.to(torch.float64), float(inertia.item())
    return torch_ref.kmeans_assign_reduce(X, C, x_sq)


# `kmeans_step_resident` limits; `_resident_lds_bytes` mirrors the extension's
# `kmeans_resident_lds_bytes(k, d)` (hip/ops.hip).
_KR_ROWS = 64
_KR_LDS_BUDGET = 160 * 1024
_KR_MAX_ACC_TILES = 8
# Whether the kernel serves the step when SRML_KMEANS_VARIANT is unset: decided
# by the alternating timings in RESULTS.md ("KMeans resident step").
_RESIDENT_DEFAULT = True


def _resident_lds_bytes(k: int, d: int) -> int:
    """LDS the resident kernel needs for (k, d); 0 where the shape is not
    legal (accumulator tiles per wave, or centres + row tile over the LDS)."""
    if k < 1 or d < 1:
        return 0
    k_pad = (k + 31) // 32 * 32
    kt, dw = k_pad // 32, ((d + 31) // 32 + 3) // 4
    if kt * dw > _KR_MAX_ACC_TILES:
        return 0
    ld = (d + 1) // 2 * 2 + 1
    lds = (k_pad + _KR_ROWS) * ld * 4 + k_pad * 8 + _KR_ROWS * 4 + 2 * _KR_ROWS * 8
    return lds if lds <= _KR_LDS_BUDGET else 0


def _resident_wanted(X: torch.Tensor, C: torch.Tensor) -> bool:
    """Route the whole step through `kmeans_step_resident`? On the GPU, for
    contiguous f32 X, k < 384 and a (k, d) whose centres and row tile fit the
    kernel's LDS. SRML_KMEANS_VARIANT=resident asks for the kernel, which it
    gets wherever it is legal; =f32 and =fused keep the small-k paths they
    name; unset, and every value that names no small-k path, follows
    `_RESIDENT_DEFAULT`."""
    variant = os.environ.get("SRML_KMEANS_VARIANT")
    if variant in ("f32", "fused"):
        return False
    if variant != "resident" and not _RESIDENT_DEFAULT:
        return False
    if not (X.is_cuda and X.dtype == torch.float32 and X.dim() == 2 and X.is_contiguous()):
        return False
    if C.dtype != torch.float32 or X.shape[0] == 0 or C.shape[0] >= 384:
        return False
    return _resident_lds_bytes(C.shape[0], X.shape[1]) > 0


def _step_resident(
    ext, X: torch.Tensor, C: torch.Tensor, x_sq: torch.Tensor
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, float]:
    """One Lloyd step in one pass over X: labels, f64 sums and counts, inertia."""
    labels, sums, counts, inertia = ext.kmeans_step_resident(
        X, C.contiguous(), x_sq.contiguous()
    )
    return labels, sums, counts, float(inertia.item())


def _step_f64(
    ext, X: torch.Tensor, C: torch.Tensor, x_sq: Optional[torch.Tensor]
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, float]:
    """One Lloyd step on f64 rows: `kmeans_assign_f64` (f64 MFMA, argmin kept
    in registers) + `label_accumulate_f64`. No floating atomics in either, so
    a repeated call returns the same bits."""
    X = X.contiguous()
    x_sq = _xsq(X) if x_sq is None else x_sq.to(torch.float64).contiguous()
    labels, _min_d, inertia = ext.kmeans_assign_f64(
        X, C.to(torch.float64).contiguous(), x_sq
    )
    sums, counts = ext.label_accumulate_f64(X, labels, C.shape[0])
    return labels, sums, counts, float(inertia.item())


def kmeans_predict(X: torch.Tensor, C: torch.Tensor) -> torch.Tensor:
    if use_hip(X) and X.dtype == torch.float64:
        X = X.contiguous()
        return hip_ops().kmeans_assign_f64(
            X, C.to(torch.float64).contiguous(), _xsq(X)
        )[0]
    if use_hip(X) and X.dtype == torch.float32:
        X = X.contiguous()
        return _assign(hip_ops(), X, C, _xsq(X))[0]
    return torch_ref.kmeans_predict(X, C)


def _assign(
    ext, X: torch.Tensor, C: torch.Tensor, x_sq: torch.Tensor
) -> Tuple[torch.Tensor, torch.Tensor]:
    """(labels, inertia) for contiguous f32 X through the k-gated dispatch.

    Measured on 100M x 128 / 1M x 3000 (profiles/README):
    - large k: [k, n] GEMM + kmeans_argmin_kn (47.6 vs 74.5 ms at k=1000 —
      the dot block is compute-shaped there); k > 16384 no longer fits the
      epilogue's LDS and takes the fused kernel
    - large k and d >= D_MIN: the same [k, n] block from the split-bf16
      screen, `_assign_split` (27.4 vs 47.4 ms per step at k=1000, d=3000)
    - small k: X @ C^T tall-skinny GEMM + kmeans_argmin_nk wave-per-row
      epilogue (the fused kernel's 2-k-step pipeline never reaches steady
      state at small d, and the [k, n] skinny-m GEMM stalls: 205 / 280 ms
      vs 66 ms at k=200)"""
    n, k = X.shape[0], C.shape[0]
    variant = os.environ.get("SRML_KMEANS_VARIANT")
    if variant == "fused" or k * 4 > 64 * 1024 or n == 0:
        labels, _min_d, inertia = ext.kmeans_assign(
            X, C.contiguous(), x_sq.contiguous()
        )
        return labels, inertia
    if k < 384:
        return _assign_gemm(ext, X, C, x_sq, n, k, layout="nk")
    if _use_split(variant, X.shape[1]):
        return _assign_split(ext, X, C, x_sq, n, k, exact=variant == "split_f64")
    return _assign_gemm(ext, X, C, x_sq, n, k, layout="kn")


def _assign_gemm(
    ext, X: torch.Tensor, C: torch.Tensor, x_sq: torch.Tensor, n: int, k: int,
    max_dots_bytes: int = 8 << 30, layout: str = "kn",
) -> Tuple[torch.Tensor, torch.Tensor]:
    """GEMM + argmin-epilogue assignment, row-chunked so the dot block stays
    under `max_dots_bytes`. layout "kn": C @ X_chunkᵀ ([k, chunk]) +
    `kmeans_argmin_kn`; "nk": tall-skinny X_chunk @ Cᵀ (row-major [chunk, k])
    + the wave-per-row `kmeans_argmin_nk`."""
    kn = layout == "kn"
    c_sq = (C * C).sum(dim=1).contiguous()
    # "nk": [d, k] so the GEMM B operand is plain N-layout
    Cm = C.contiguous() if kn else C.t().contiguous()
    argmin = ext.kmeans_argmin_kn if kn else ext.kmeans_argmin_nk

    def dots_of(s: int, e: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        return torch.mm(Cm, X[s:e].T, out=out) if kn else torch.mm(X[s:e], Cm, out=out)

    def dots_buf(m: int) -> torch.Tensor:
        return torch.empty((k, m) if kn else (m, k), dtype=torch.float32, device=X.device)

    rchunk = max(256, int(max_dots_bytes // max(1, k * 4)))
    if rchunk >= n:
        labels, _min_d, inertia = argmin(dots_of(0, n), x_sq, c_sq)
        return labels, inertia
    labels = torch.empty(n, dtype=torch.int32, device=X.device)
    inertia = torch.zeros(1, dtype=torch.float64, device=X.device)
    dots = dots_buf(rchunk)
    for s in range(0, n, rchunk):
        e = min(n, s + rchunk)
        dv = dots_of(s, e, out=dots if e - s == rchunk else dots_buf(e - s))
        lb, _md, it = argmin(dv, x_sq[s:e].contiguous(), c_sq)
        labels[s:e] = lb
        inertia += it
    return labels, inertia


# Split-bf16 screen (see `_assign_split`). SPLIT_EPS bounds one screened dot's
# error relative to |x'||c'|: the three-term split is within 3*2^-18, the rest
# (~2.7x) is left for the f32 accumulation.
SPLIT_EPS = 2.0 ** -15
# Measured with tools/time_assign_split.py at 1M rows, k=1000 (tables in
# profiles/README.md). D_MIN: the screen loses at d=256 (5.29 vs 4.95 ms) and
# wins at d=512 (6.55 vs 8.22 ms); below that the split pass and the second
# pass over the dot block outweigh the cheaper GEMM. F_MAX: the screen still
# wins 1.48x at 12.8 % flagged and breaks even near 40 % (`_refine_f32` costs
# about 50 ns per flagged row); a fallback costs the discarded screen of one
# chunk on top of the f32 path, so the cut-off sits below the break-even.
D_MIN = 512
F_MAX = 0.25


def _use_split(variant: Optional[str], d: int) -> bool:
    """SRML_KMEANS_VARIANT=f32 forces the f32 GEMM, =split and =split_f64
    (near-ties decided in f64) force the screen; unset takes the screen from
    D_MIN columns on."""
    if variant == "f32":
        return False
    return variant in ("split", "split_f64") or d >= D_MIN


def _split_dots(
    Ch2: torch.Tensor, Cl: torch.Tensor, SX: torch.Tensor, dp: int, out: torch.Tensor
) -> torch.Tensor:
    """out[k, m] = Ch·Xh + Ch·Xl + Cl·Xh from the split operands: bf16 in, f32
    accumulate, f32 out (a bf16 result would discard what the split buys).
    [Ch|Ch] @ [Xh|Xl]ᵀ, then += Cl @ Xhᵀ on the strided hi half (no copy)."""
    torch.mm(Ch2, SX.T, out_dtype=torch.float32, out=out)
    return torch.addmm(out, Cl, SX[:, :dp].T, out_dtype=torch.float32, out=out)


def _fallback_f32(
    ext, X: torch.Tensor, C: torch.Tensor, x_sq: torch.Tensor, n: int, k: int
) -> Tuple[torch.Tensor, torch.Tensor]:
    """The screen separated too few rows (duplicate / degenerate centres):
    this call runs the f32 GEMM path instead."""
    return _assign_gemm(ext, X, C, x_sq, n, k, layout="kn")


def _refine_f32(
    ext, Xc: torch.Tensor, C: torch.Tensor, x_sqc: torch.Tensor, rows: torch.Tensor
) -> Tuple[torch.Tensor, torch.Tensor]:
    """(labels, inertia) of the listed rows of Xc by the f32 path's own
    arithmetic: the f32 library GEMM on the gathered rows + `kmeans_argmin_kn`.

    A near-tie is decided by rounding, so only the same rounding reproduces
    what the f32 path assigns. Per element the library GEMM walks K in one
    order whatever the shape, except in the few tiles it splits along K:
    gathered rows, padded to a multiple of 256 with repeats of the first one,
    get 97-100 % of their dots bit-equal to the full GEMM's (measured,
    profiles/README.md), against 3 % unpadded at 64 rows or fewer."""
    nf = rows.numel()
    pad = -nf % 256
    idx = torch.cat([rows, rows[:1].expand(pad)]) if pad else rows
    dots = torch.mm(C, Xc[idx].T)
    c_sq = (C * C).sum(dim=1).contiguous()
    lf, md, _it = ext.kmeans_argmin_kn(dots, x_sqc[idx].contiguous(), c_sq)
    return lf[:nf], md[:nf].double().sum()


def _assign_split(
    ext, X: torch.Tensor, C: torch.Tensor, x_sq: torch.Tensor, n: int, k: int,
    max_bytes: int = 8 << 30, exact: bool = False,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Screened assignment: the [k, chunk] dot block comes from the bf16 MFMA
    rate instead of the f32 one, and only near-ties are decided again.

    X and C are centred by the column mean of C (distances are translation
    invariant; without it data far from the origin flags every row) and split
    by `kmeans_split_bf16` into bf16 hi|lo halves; `_split_dots` forms the
    three-term product, each dot within SPLIT_EPS·|x'||c'| of exact.
    `kmeans_argmin_kn_screen` finalises every row whose best two values are
    further apart than 4·SPLIT_EPS·|x'|·max|c'| — there the screen's argmin is
    the exact one and, its rounding being far smaller than that margin, the f32
    path's too — and lists the others. Those are
    decided by `_refine_f32`, as the f32 path decides them, so a fit takes the
    course it took before; with `exact` (SRML_KMEANS_VARIANT=split_f64)
    `kmeans_refine` decides them in f64 from the original X and C instead,
    and labels equal the f64 argmin wherever the bound holds. Rows are chunked
    so split buffer + dot block stay under `max_bytes`. If more than F_MAX of
    a chunk is listed, the screen is discarded and `_fallback_f32` runs the
    call."""
    Cc = C.contiguous()
    mu = Cc.mean(dim=0)
    SC, c_sq = ext.kmeans_split_bf16(Cc, mu)
    dp = SC.shape[1] // 2
    Ch2 = torch.cat([SC[:, :dp], SC[:, :dp]], dim=1)
    Cl = SC[:, dp:].contiguous()
    margin = ((4.0 * SPLIT_EPS) * c_sq.max().sqrt()).reshape(1)

    rchunk = max(256, int(max_bytes // (k * 4 + 4 * dp)))
    single = rchunk >= n
    labels = None if single else torch.empty(n, dtype=torch.int32, device=X.device)
    inertia = torch.zeros(1, dtype=torch.float64, device=X.device)
    dots = torch.empty((k, min(n, rchunk)), dtype=torch.float32, device=X.device)
    for s in range(0, n, rchunk):
        e = min(n, s + rchunk)
        Xc = X[s:e]
        SX, a_sq = ext.kmeans_split_bf16(Xc, mu)
        if e - s != dots.shape[1]:
            dots = torch.empty((k, e - s), dtype=torch.float32, device=X.device)
        _split_dots(Ch2, Cl, SX, dp, dots)
        del SX  # only the GEMMs read it; the next chunk's split reuses the block
        lb, md, it, flagged, n_flagged = ext.kmeans_argmin_kn_screen(
            dots, a_sq, c_sq, margin
        )
        nf = int(n_flagged.item())
        if nf > F_MAX * (e - s):
            return _fallback_f32(ext, X, C, x_sq, n, k)
        if nf and exact:
            ext.kmeans_refine(
                Xc, Cc, dots, c_sq, a_sq, margin, flagged, n_flagged, lb, md, it
            )
        elif nf:
            rows = flagged[:nf].long()
            lf, itf = _refine_f32(ext, Xc, Cc, x_sq[s:e], rows)
            lb[rows] = lf
            it += itf
        if single:
            return lb, it
        labels[s:e] = lb
        inertia += it
    return labels, inertia


# One-term screen on the prepared hi plane (see `_assign_prepared`). With
# u = 2^-9, hi·hi differs from the three-term product by at most
# (2u + u²)·Σ|x'ᵢc'ᵢ| <= 2^-8 (1 + 2^-10) |x'||c'|, and SPLIT_EPS covers the
# three-term product's own error with room for that 2^-18.
EPS_HI = 2.0 ** -8 + SPLIT_EPS
# Share of a chunk the hi screen may flag before the chunk falls up to the
# three-term screen. Measured at 1M x 3000, k=1000 (tools/time_assign_split.py
# --prepared; table in profiles/README.md): a fall-up costs 15.4 ms (split of
# X 4.9, K=2·dp addmm 9.8, second screen 0.7), `_refine_f32` 51 to 71 ns per
# flagged row, so the two meet near 28 % flagged; the cut-off sits below that.
F_HI = 0.20


class _Prepared:
    """What a fit reuses of X: the centring point, the bf16 hi plane of X - mu
    ([n, dp], zero pad columns) and |x - mu|², plus the key they belong to.

    And what `_accumulate_delta` carries from step to step, valid while
    `k` != 0: `prev`, a private copy of the last labels; the anchors `R`
    (f32 [k, d], the centres of the last full pass); and the per-centre
    moments about them in f64, `cnt` [k], `S` = Σ(x − r) [k, d] and
    `Q` = Σ|x − r|² [k]; `E` [k, d] is what the f32 Σx of that full pass
    differed from S + cnt·R by. They depend on the labels alone, never on C.

    And the reference state of the row bounds (`_assign_bounded`), valid while
    `ref_k` != 0: `C_ref`, a private copy of the centres of the last reference
    pass; `lab_ref` (i32 [n]), its final labels; and `gap_ref` (f32 [n]), per
    row a certified lower bound of (second − best) of |c'_j|² − 2x'·c'_j at
    those centres, 0 where the row was a near-tie. `changed` is the number of
    rows whose label changed at the last step, as `_accumulate_delta` read it
    (n where it did not, 0 on an entry it has not seen)."""

    __slots__ = ("ref", "key", "mu", "H", "a_sq", "finalizer",
                 "k", "prev", "R", "S", "cnt", "Q", "E",
                 "ref_k", "C_ref", "lab_ref", "gap_ref", "changed")


_PREP: Optional[_Prepared] = None


def _key(X: torch.Tensor) -> tuple:
    return (X._version, X.data_ptr(), tuple(X.shape))


def _drop_prepared(token: Optional[_Prepared] = None) -> None:
    """Empties the cache; with `token`, only if it still holds that entry."""
    global _PREP
    if token is None or _PREP is token:
        if _PREP is not None:
            _PREP.finalizer.detach()
        _PREP = None


def _cache_applies(X: torch.Tensor, C: torch.Tensor) -> bool:
    """The gates of `_assign` that lead to `_assign_split`, for a contiguous
    device X, unless SRML_KMEANS_CACHE=0."""
    if os.environ.get("SRML_KMEANS_CACHE") == "0":
        return False
    if not (X.is_cuda and X.is_contiguous() and X.dim() == 2):
        return False
    n, k = X.shape[0], C.shape[0]
    variant = os.environ.get("SRML_KMEANS_VARIANT")
    if variant in ("f32", "fused") or k * 4 > 64 * 1024 or n == 0 or k < 384:
        return False
    return _use_split(variant, X.shape[1])


def _prepared(ext, X: torch.Tensor, C: torch.Tensor) -> Optional[_Prepared]:
    """The cache entry of X, built against the column mean of this C if X is
    new (so the first call centres as `_assign_split` does). None, and today's
    path, if the entry would take more than a quarter of the free device
    memory. Dropped when X is collected, when another X or a modified X comes
    in, and when a call ends in `_fallback_f32` (the next one re-centres)."""
    global _PREP
    p = _PREP
    if p is not None and p.ref() is X and p.key == _key(X):
        return p
    _drop_prepared()
    n, d = X.shape
    dp = (d + 31) // 32 * 32
    free, _total = torch.cuda.mem_get_info(X.device)
    if n * dp * 2 + n * 4 > free // 4:
        return None
    p = _Prepared()
    p.mu = C.contiguous().mean(dim=0)
    p.H, p.a_sq = ext.kmeans_split_bf16_hi(X, p.mu)
    p.ref = weakref.ref(X)
    p.key = _key(X)
    p.finalizer = weakref.finalize(X, _drop_prepared, p)
    p.k = 0
    p.prev = p.R = p.S = p.cnt = p.Q = p.E = None
    p.ref_k = p.changed = 0
    p.C_ref = p.lab_ref = p.gap_ref = None
    _PREP = p
    return p


# Share of the rows that may change label before a step takes the full pass
# instead of the delta (see `_accumulate_delta`). Measured at 1M x 3000, k=1000
# (tools/time_kmeans_delta.py; table in profiles/README.md "Delta step"): the
# delta path takes 0.40 ms at 1 % changed, 1.04 at 10 %, 1.89 at 25 % and 3.30
# at 50 % against 2.9 ms for the full pass; they cross near 40 %.
F_DELTA = 0.25
# Form of `kmeans_delta_accumulate`: entries sorted by label and streamed per
# segment, or one block per entry with an f64 atomic per column (faster only
# below 0.5 % changed, by 0.08 ms; 3.6 against 1.0 ms at 10 %).
DELTA_SORTED = True


def _accumulate_delta(
    ext, X: torch.Tensor, labels: torch.Tensor, C: torch.Tensor, prep: _Prepared
) -> Tuple[torch.Tensor, torch.Tensor, float]:
    """(sums f64 [k,d], counts f64 [k], inertia) of `labels`, from the rows
    that changed label since the last call on this entry where it can.

    The entry keeps n_j, S_j = Σ(x − r_j) and Q_j = Σ|x − r_j|² per centre
    about the anchors r_j, the centres of the last full pass. Then
    Σx = S_j + n_j r_j and Σ|x − c_j|² = Q_j − 2(c_j − r_j)·S_j + n_j|c_j − r_j|²
    (`kmeans_anchor_inertia`), and a row that moves from one label to another
    leaves the one and enters the other as a direct difference against their
    anchors (`kmeans_label_delta`, `kmeans_delta_accumulate`): X is read at
    the changed rows only. Full pass (`label_accumulate_inertia` with
    `anchor`, which also re-anchors at C) when the entry holds no moments for
    this k, when more than F_DELTA of the rows changed, and when the drift
    D = Σ n_j|c_j − r_j|² exceeds ΣQ_j, the correction terms then being no
    longer small beside what they correct. What is returned never aliases
    the kept state, nor the state the caller's labels."""
    n, k = X.shape[0], C.shape[0]
    Cc = C.contiguous()
    prep.changed = n  # not known on a fresh entry or another k
    if prep.k == k:
        ent_lab, ent_row, n_changed = ext.kmeans_label_delta(labels, prep.prev)
        m = prep.changed = int(n_changed.item())
        if m <= F_DELTA * n:
            if m:
                ext.kmeans_delta_accumulate(
                    X, ent_lab, ent_row, n_changed, m, prep.R, prep.S, prep.cnt, prep.Q,
                    DELTA_SORTED,
                )
            out, sums = ext.kmeans_anchor_inertia(
                Cc, prep.R, prep.S, prep.cnt, prep.Q, prep.E
            )
            inertia, drift, q_sum = out.tolist()
            if not drift > q_sum:
                return sums, prep.cnt.clone(), inertia
    sums, counts, inertia, Q, dsums = ext.label_accumulate_inertia(
        X, labels, Cc, anchor=True
    )
    sums = sums.to(torch.float64)
    prep.prev = labels.clone()
    prep.R = Cc.clone()
    prep.S, prep.cnt, prep.Q, prep.k = dsums.to(torch.float64), counts.to(torch.float64), Q, k
    # S is kept about R so that Σ(x − r) does not carry the f32 rounding of Σx
    # far from the origin; E ties the sums returned from now on to this Σx
    prep.E = sums - torch.addcmul(prep.S, prep.cnt[:, None], Cc.to(torch.float64))
    return sums, prep.cnt.clone(), float(inertia.item())


# Row bounds (see `_assign_bounded`). BOUND_SLACK is `slack_rel` of
# `kmeans_bound_test`, derived above that kernel (hip/ops.hip).
BOUND_SLACK = 2.0 ** -10
# Share of the rows the bound test may leave active before the step is a
# reference pass instead. Measured at 1M x 3000, k=1000
# (tools/time_kmeans_bounds.py; table in profiles/README.md "Row bounds"):
# the active path takes 1.47 ms with the 1 % near-ties alone, 1.91 at 5 % more,
# 2.30 at 10 %, 3.54 at 25 % and 5.54 at 50 % against 6.8 ms for the full
# screen. They would cross past 60 %; the cut-off stays at its starting value,
# a step over it being one whose centres still move, where a new reference is
# worth more than the step saved.
F_SKIP = 0.25
# The bound test is tried only if at most this share of the rows changed
# label at the last step. A test that fails costs 0.4 to 0.6 ms on top of the
# reference pass that follows (`kmeans_bound_test` alone 0.50 ms); in the same
# course it failed after every step that changed 0.26 % of the labels or more
# (576k rows active after that one) and passed after 0.02 % (132k active).
F_TRY = 0.001


def _assign_bounded(
    ext, X: torch.Tensor, Cc: torch.Tensor, x_sq: torch.Tensor, prep: _Prepared,
    Ch: torch.Tensor, c_sq: torch.Tensor, margin_hi: torch.Tensor, exact: bool,
) -> Optional[torch.Tensor]:
    """Labels of this step from the reference state of the entry, or None if
    more than F_SKIP of the rows need their scores (a reference pass follows).

    With v_j = |c'_j|² − 2x'·c'_j, a move of the centres from C_ref to C
    raises v_a by at most Δ_a + 2rδ_a and lowers any other v_j by at most
    −(Δ_j − 2rδ_j) (Δ_j = |c'_j|² − |c'_ref,j|², δ_j = |c_j − c_ref,j|,
    r = |x'|: `kmeans_centre_drift`). A row whose certified gap at C_ref
    exceeds the sum of the two (`kmeans_bound_test`) still has its reference
    label as strict argmin and needs no dot product. The other, active rows
    take today's path on their own: their rows of the hi plane gathered
    (`kmeans_gather_rows_bf16`), the hi·hi GEMM, the screen, and its near-ties
    decided as `_assign_prepared` decides them. The reference state is not
    rewritten, so every step is tested against the same reference, and the
    returned labels never alias it."""
    n = X.shape[0]
    Delta, delta = ext.kmeans_centre_drift(Cc, prep.C_ref, prep.mu)
    active, n_active = ext.kmeans_bound_test(
        prep.gap_ref, prep.lab_ref, prep.a_sq, Delta, delta, BOUND_SLACK
    )
    m = int(n_active.item())
    if m > F_SKIP * n:
        return None
    labels = prep.lab_ref.clone()
    if m == 0:
        return labels
    rows = active[:m].long()
    Hg = ext.kmeans_gather_rows_bf16(prep.H, active, m)
    dots = torch.mm(Ch, Hg.T, out_dtype=torch.float32)
    a_sq = prep.a_sq[rows]
    lb, md, it, flagged, n_flagged = ext.kmeans_argmin_kn_screen(dots, a_sq, c_sq, margin_hi)
    nf = int(n_flagged.item())
    if nf and exact:
        ext.kmeans_refine(
            X[rows], Cc, dots, c_sq, a_sq, margin_hi, flagged, n_flagged, lb, md, it
        )
    elif nf:
        near = flagged[:nf].long()
        lf, _itf = _refine_f32(ext, X, Cc, x_sq, rows[near])
        lb[near] = lf
    labels[rows] = lb
    return labels


def _assign_prepared(
    ext, X: torch.Tensor, C: torch.Tensor, x_sq: torch.Tensor, prep: _Prepared,
    max_dots_bytes: int = 8 << 30, exact: bool = False,
) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Two-stage screened assignment on the prepared hi plane: (labels, None),
    the inertia being left to `label_accumulate_inertia`.

    C is split against the cached mu (any fixed centring point keeps the
    guarantee; mu is where C was when the entry was built). Per row chunk the
    hi·hi dots, each within EPS_HI·|x'||c'| of exact, are screened with margin
    4·EPS_HI·|x'|·max|c'|. At most F_HI of the chunk flagged: those rows are
    decided as `_assign_split` decides its near-ties. More: the chunk falls
    up — it is split in full against the same mu, `addmm` adds hi·lo + lo·hi
    onto the same dot block, and it goes on exactly as `_assign_split` does
    from its screen, F_MAX and `_fallback_f32` included; then the cache is
    dropped and the result is (labels, inertia) of the f32 path.

    Unless SRML_KMEANS_BOUNDS=0, a pass that screens every row is also the
    reference pass of the row bounds: it leaves `C_ref`, `lab_ref` and
    `gap_ref` on the entry (the screen's gap output; a chunk that fell up
    keeps the gap of its three-term screen), and while the entry holds them
    for this k, `_assign_bounded` is asked first."""
    n, k = X.shape[0], C.shape[0]
    Cc = C.contiguous()
    mu, H = prep.mu, prep.H
    SC, c_sq = ext.kmeans_split_bf16(Cc, mu)
    dp = SC.shape[1] // 2
    Ch = SC[:, :dp].contiguous()
    ClCh = None
    c_max = c_sq.max().sqrt()
    margin_hi = ((4.0 * EPS_HI) * c_max).reshape(1)

    bounds = os.environ.get("SRML_KMEANS_BOUNDS") != "0"
    if bounds and prep.ref_k == k and prep.changed <= F_TRY * n:
        labels = _assign_bounded(ext, X, Cc, x_sq, prep, Ch, c_sq, margin_hi, exact)
        if labels is not None:
            return labels, None
    prep.ref_k = 0  # rewritten below, or stale
    gap = torch.empty(n, dtype=torch.float32, device=X.device) if bounds else None

    rchunk = max(256, int(max_dots_bytes // (k * 4)))
    single = rchunk >= n
    labels = None if single else torch.empty(n, dtype=torch.int32, device=X.device)
    dots = torch.empty((k, min(n, rchunk)), dtype=torch.float32, device=X.device)
    for s in range(0, n, rchunk):
        e = min(n, s + rchunk)
        Xc = X[s:e]
        a_sq = prep.a_sq[s:e]
        if e - s != dots.shape[1]:
            dots = torch.empty((k, e - s), dtype=torch.float32, device=X.device)
        torch.mm(Ch, H[s:e].T, out_dtype=torch.float32, out=dots)
        margin = margin_hi
        gap_kw = {"gap_out": gap[s:e]} if bounds else {}
        lb, md, it, flagged, n_flagged = ext.kmeans_argmin_kn_screen(
            dots, a_sq, c_sq, margin, **gap_kw
        )
        nf = int(n_flagged.item())
        if nf > F_HI * (e - s):
            if ClCh is None:
                ClCh = torch.cat([SC[:, dp:], SC[:, :dp]], dim=1)
            SX, _a = ext.kmeans_split_bf16(Xc, mu)
            # [Cl|Ch] @ [Xh|Xl]ᵀ = Cl·Xh + Ch·Xl, onto the hi·hi already there
            torch.addmm(dots, ClCh, SX.T, out_dtype=torch.float32, out=dots)
            del SX
            margin = ((4.0 * SPLIT_EPS) * c_max).reshape(1)
            lb, md, it, flagged, n_flagged = ext.kmeans_argmin_kn_screen(
                dots, a_sq, c_sq, margin, **gap_kw
            )
            nf = int(n_flagged.item())
            if nf > F_MAX * (e - s):
                _drop_prepared()
                return _fallback_f32(ext, X, C, x_sq, n, k)
        if nf and exact:
            ext.kmeans_refine(
                Xc, Cc, dots, c_sq, a_sq, margin, flagged, n_flagged, lb, md, it
            )
        elif nf:
            rows = flagged[:nf].long()
            lf, _itf = _refine_f32(ext, Xc, Cc, x_sq[s:e], rows)
            lb[rows] = lf
        if single:
            labels = lb
        else:
            labels[s:e] = lb
    if bounds:
        prep.C_ref, prep.lab_ref, prep.gap_ref, prep.ref_k = Cc.clone(), labels.clone(), gap, k
    return labels, None


def _xsq(X: torch.Tensor) -> torch.Tensor:
    return (X * X).sum(dim=1)
