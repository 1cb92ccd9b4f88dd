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

Across the calls of one fit X does not change, so `kmeans_assign_reduce`
keeps the centred bf16 hi plane of X and |x'|² (`_prepared`, one entry,
SRML_KMEANS_CACHE=0 disables it) and screens with the hi·hi term alone
(`_assign_prepared`): one K=dp GEMM instead of three terms and no split pass
over X. A chunk with too many near-ties adds the other two terms onto the
same dot block. That path reports the inertia `label_accumulate_inertia`
sums beside the accumulation, as (x − c)² directly.

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
    SRML_KMEANS_CACHE=0 turns the cache off."""
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
                    sums, counts, inertia = ext.label_accumulate_inertia(
                        X, labels, C.contiguous()
                    )
                else:  # ended in `_fallback_f32`
                    sums, counts = ext.label_accumulate(X, labels, C.shape[0])
                return (labels, sums.to(torch.float64), counts.to(torch.float64),
                        float(inertia.item()))
        X = X.contiguous()
        labels, inertia = _assign(ext, X, C, x_sq)
        sums, counts = ext.label_accumulate(X, labels, C.shape[0])
        return labels, sums.to(torch.float64), counts.to(torch.float64), float(inertia.item())
    return torch_ref.kmeans_assign_reduce(X, C, x_sq)


def kmeans_predict(X: torch.Tensor, C: torch.Tensor) -> torch.Tensor:
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
    ([n, dp], zero pad columns) and |x - mu|², plus the key they belong to."""

    __slots__ = ("ref", "key", "mu", "H", "a_sq", "finalizer")


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
    _PREP = p
    return p


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
    dropped and the result is (labels, inertia) of the f32 path."""
    n, k = X.shape[0], C.shape[0]
    Cc = C.contiguous()
    mu, H = prep.mu, prep.H
    SC, c_sq = ext.kmeans_split_bf16(Cc, mu)
    dp = SC.shape[1] // 2
    Ch = SC[:, :dp].contiguous()
    ClCh = None
    c_max = c_sq.max().sqrt()
    margin_hi = ((4.0 * EPS_HI) * c_max).reshape(1)

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
        lb, md, it, flagged, n_flagged = ext.kmeans_argmin_kn_screen(
            dots, a_sq, c_sq, margin
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
                dots, a_sq, c_sq, margin
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
            return lb, None
        labels[s:e] = lb
    return labels, None


def _xsq(X: torch.Tensor) -> torch.Tensor:
    return (X * X).sum(dim=1)
