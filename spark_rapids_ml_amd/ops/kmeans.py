"""KMeans ops: fused assignment (MFMA distance + argmin) + accumulation.

HIP path (gfx950): `kmeans_assign` — LDS-tiled ‖x‖²+‖c‖²−2x·c with the
−2XCᵀ term on mfma_f32_32x32x2f32, fused per-row argmin (packed 64-bit
atomicMin) and block-reduced inertia; `label_accumulate` — vectorized
per-center sum/count scatter. Together these are the KMeansMG Lloyd-step
kernel family of the reference (clustering.py:381-415).
"""

from __future__ import annotations

import os
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

    Default GPU path: hipBLASLt GEMM for the C @ Xᵀ dot block (141 TF on the
    1M×3000×k=1000 headline shape) + the own `kmeans_argmin_kn` epilogue
    (one bandwidth-bound pass) + `label_accumulate`. The all-in-one MFMA
    `kmeans_assign` kernel (84 TF, profiles/README.md ladder) stays selected
    via SRML_KMEANS_VARIANT=fused."""
    if use_hip(X) and X.dtype == torch.float32:
        ext = hip_ops()
        X = X.contiguous()
        labels, inertia = _assign(ext, X, C, _xsq(X) if x_sq is None else x_sq)
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
    - small k: X @ C^T tall-skinny GEMM + kmeans_argmin_nk wave-per-row
      epilogue (the fused kernel's 2-k-step pipeline never reaches steady
      state at small d, and the [k, n] skinny-m GEMM stalls: 205 / 280 ms
      vs 66 ms at k=200)"""
    n, k = X.shape[0], C.shape[0]
    fused = os.environ.get("SRML_KMEANS_VARIANT") == "fused"
    if fused or k * 4 > 64 * 1024 or n == 0:
        labels, _min_d, inertia = ext.kmeans_assign(
            X, C.contiguous(), x_sq.contiguous()
        )
        return labels, inertia
    return _assign_gemm(ext, X, C, x_sq, n, k, layout="kn" if k >= 384 else "nk")


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


def _xsq(X: torch.Tensor) -> torch.Tensor:
    return (X * X).sum(dim=1)
