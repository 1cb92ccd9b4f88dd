"""Pure-torch fp32/fp64 reference implementations of every HIP op.

These are the numerics oracles GPU tests compare the HIP kernels against,
and the execution path on CPU-only machines. They are written chunked so the
CPU test path stays memory-bounded on large inputs.
"""

from __future__ import annotations

from typing import Any, Optional, Tuple

import torch


def kmeans_assign_reduce(
    X: torch.Tensor,
    C: torch.Tensor,
    x_sq: Optional[torch.Tensor] = None,
    chunk: int = 65536,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, float]:
    """Fused Lloyd step (assignment + per-center accumulation).

    Returns (labels int32 [n], sums f64 [k,d], counts f64 [k], inertia).
    Distance: squared euclidean via ||x||^2 + ||c||^2 - 2 x.c (the HIP kernel
    computes the same expansion with the -2XC^T term on MFMA).
    """
    n, d = X.shape
    k = C.shape[0]
    dev = X.device
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    sums = torch.zeros((k, d), dtype=torch.float64, device=dev)
    counts = torch.zeros(k, dtype=torch.float64, device=dev)
    inertia = torch.zeros((), dtype=torch.float64, device=dev)
    if n == 0:
        return labels, sums, counts, 0.0
    c_sq = (C.to(torch.float32) ** 2).sum(dim=1)
    if x_sq is None:
        x_sq = (X.to(torch.float32) ** 2).sum(dim=1)
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        xb = X[s:e]
        dist = x_sq[s:e, None] + c_sq[None, :] - 2.0 * (xb @ C.T)
        md, lb = dist.min(dim=1)
        labels[s:e] = lb.to(torch.int32)
        sums.index_add_(0, lb, xb.to(torch.float64))
        counts.index_add_(0, lb, torch.ones_like(md, dtype=torch.float64))
        inertia += torch.clamp(md, min=0).to(torch.float64).sum()
    return labels, sums, counts, float(inertia.item())


def kmeans_predict(
    X: torch.Tensor, C: torch.Tensor, chunk: int = 65536
) -> torch.Tensor:
    n = X.shape[0]
    labels = torch.empty(n, dtype=torch.int32, device=X.device)
    if n == 0:
        return labels
    c_sq = (C**2).sum(dim=1)
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        xb = X[s:e]
        dist = c_sq[None, :] - 2.0 * (xb @ C.T)
        labels[s:e] = dist.argmin(dim=1).to(torch.int32)
    return labels


def gram(X: torch.Tensor) -> torch.Tensor:
    """X^T X in fp32 (or the input dtype if f64)."""
    return X.T @ X


def xty(X: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    return X.T @ y


def pairwise_sq_dists(
    X: torch.Tensor, Y: torch.Tensor
) -> torch.Tensor:
    x_sq = (X**2).sum(dim=1)
    y_sq = (Y**2).sum(dim=1)
    return torch.clamp(x_sq[:, None] + y_sq[None, :] - 2.0 * (X @ Y.T), min=0.0)


def knn_topk(
    Q: torch.Tensor,
    I: torch.Tensor,
    k: int,
    chunk: int = 8192,
    item_chunk_elems: int = 1 << 31,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Brute-force kNN of queries Q against items I: returns (dists [q,k],
    idx int64 [q,k]) with squared-euclid computed f32 then sqrt'ed.
    Items are chunked too (running top-k merge) so the distance block stays
    bounded — 10M items × an 8k query chunk would otherwise materialize
    hundreds of GB."""
    nq, ni = Q.shape[0], I.shape[0]
    k = min(k, ni)
    dists = torch.empty((nq, k), dtype=torch.float32, device=Q.device)
    idx = torch.empty((nq, k), dtype=torch.int64, device=Q.device)
    ichunk = max(k, min(ni, item_chunk_elems // max(1, chunk)))
    for s in range(0, nq, chunk):
        e = min(nq, s + chunk)
        qb = Q[s:e]
        q_sq = (qb**2).sum(dim=1)[:, None]
        best_d: torch.Tensor = None  # type: ignore[assignment]
        best_i: torch.Tensor = None  # type: ignore[assignment]
        for s2 in range(0, ni, ichunk):
            e2 = min(ni, s2 + ichunk)
            ib = I[s2:e2]
            d2 = q_sq + (ib**2).sum(dim=1)[None, :] - 2.0 * (qb @ ib.T)
            kk = min(k, e2 - s2)
            vals, ids = torch.topk(d2, kk, dim=1, largest=False)
            ids = ids + s2
            if best_d is None:
                best_d, best_i = vals, ids
            else:
                cat_d = torch.cat([best_d, vals], dim=1)
                cat_i = torch.cat([best_i, ids], dim=1)
                best_d, order = torch.topk(cat_d, min(k, cat_d.shape[1]), dim=1, largest=False)
                best_i = cat_i.gather(1, order)
        if best_d.shape[1] < k:  # ni < k edge
            pad = k - best_d.shape[1]
            best_d = torch.nn.functional.pad(best_d, (0, pad), value=float("inf"))
            best_i = torch.nn.functional.pad(best_i, (0, pad), value=-1)
        dists[s:e] = torch.sqrt(torch.clamp(best_d, min=0.0))
        idx[s:e] = best_i
    return dists, idx


# metrics that are per-coordinate reductions (no GEMM form) and the ones that
# reduce to a dot product of preprocessed rows; canonical names only, the
# alias table lives in ops/knn.py
TILE_METRICS = ("manhattan", "chebyshev", "minkowski", "canberra", "hamming")
GEMM_METRICS = ("sqeuclidean", "cosine", "correlation", "hellinger")


def metric_rows(X: torch.Tensor, metric: str) -> torch.Tensor:
    """Rows preprocessed so that a GEMM-family distance is 1 - <x', y'>:
    unit rows (cosine), centred unit rows (correlation), sqrt rows (hellinger).
    Raises ValueError where the metric is undefined for a row."""
    if metric == "hellinger":
        if bool((X < 0).any()):
            raise ValueError("metric='hellinger' requires non-negative inputs")
        return torch.sqrt(X)
    if metric == "correlation":
        X = X - X.mean(dim=1, keepdim=True)
    elif metric != "cosine":
        raise ValueError(f"metric {metric!r} has no row transform")
    norm = torch.sqrt((X * X).sum(dim=1, keepdim=True))
    if bool((norm == 0).any()):
        what = "zero-norm rows" if metric == "cosine" else "constant rows"
        raise ValueError(f"metric={metric!r} is undefined for {what}")
    # a true division: scaling a row by 2^j scales its norm by exactly 2^j,
    # so the unit row is bit-identical
    return X / norm


def _tile_keys(Q: torch.Tensor, I: torch.Tensor, metric: str, p: float) -> torch.Tensor:
    """[q, n] monotone keys of a tile metric (sum, max, sum |.|^p, mismatch
    count) through a [q, n, d] broadcast; the caller bounds q * n * d."""
    if metric == "hamming":
        return (Q[:, None, :] != I[None, :, :]).sum(dim=2).to(torch.float32)
    diff = (Q[:, None, :] - I[None, :, :]).abs()
    if metric == "manhattan":
        return diff.sum(dim=2)
    if metric == "chebyshev":
        return diff.amax(dim=2)
    if metric == "minkowski":
        return (diff ** p).sum(dim=2)
    if metric == "canberra":
        den = Q.abs()[:, None, :] + I.abs()[None, :, :]
        return torch.where(den > 0, diff / den, torch.zeros_like(diff)).sum(dim=2)
    raise ValueError(f"unknown tile metric {metric!r}")


def finish_keys(keys: torch.Tensor, metric: str, p: float, d: int) -> torch.Tensor:
    """Monotone keys -> distances (applied to the k survivors only)."""
    if metric == "minkowski":
        return keys ** (1.0 / p)
    if metric == "hamming":
        # in f64: a division by a host scalar may run as a multiplication by
        # its reciprocal, which in f32 is not the correctly rounded count / d
        return (keys.to(torch.float64) / float(d)).to(torch.float32)
    if metric in ("cosine", "correlation", "sqeuclidean"):
        return torch.clamp(keys, min=0.0)
    if metric == "hellinger":
        return torch.sqrt(torch.clamp(keys, min=0.0))
    if metric == "jaccard":
        return keys  # the key is the distance
    return keys


def _metric_keys(Q: torch.Tensor, I: torch.Tensor, metric: str, p: float,
                 block_elems: int = 1 << 24) -> torch.Tensor:
    """[q, n] keys of PREPROCESSED rows; the [rows, n, d] intermediate of the
    tile metrics is bounded by block_elems."""
    if metric == "sqeuclidean":
        return pairwise_sq_dists(Q, I)
    if metric in GEMM_METRICS:
        return 1.0 - Q @ I.T
    n, d = I.shape[0], max(1, I.shape[1])
    rows = max(1, block_elems // max(1, n * d))
    out = torch.empty((Q.shape[0], n), dtype=torch.float32, device=Q.device)
    for s in range(0, Q.shape[0], rows):
        out[s:s + rows] = _tile_keys(Q[s:s + rows], I, metric, p)
    return out


def pairwise_distances(
    Q: torch.Tensor, I: torch.Tensor, metric: str = "euclidean", p: float = 2.0
) -> torch.Tensor:
    """[q, n] f32 distances under a canonical metric name (scipy cdist
    definitions; hellinger is sqrt(max(0, 1 - sum sqrt(x_i y_i))))."""
    if metric == "euclidean":
        return torch.sqrt(pairwise_sq_dists(Q, I))
    if metric in ("cosine", "correlation", "hellinger"):
        Q, I = metric_rows(Q, metric), metric_rows(I, metric)
    elif metric not in TILE_METRICS and metric != "sqeuclidean":
        raise ValueError(f"unknown metric {metric!r}")
    return finish_keys(_metric_keys(Q, I, metric, p), metric, p, I.shape[1])


def knn_topk_metric(
    Q: torch.Tensor,
    I: torch.Tensor,
    k: int,
    metric: str = "euclidean",
    p: float = 2.0,
    block_elems: int = 1 << 24,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Brute-force kNN under a canonical metric: (dists [q,k] ascending, idx
    int64 [q,k]). Queries and items are both chunked with a running top-k
    merge, so no block larger than block_elems elements ([q, n] for the GEMM
    family, [q, n, d] for the tile family) is ever materialized."""
    if metric == "euclidean":
        return knn_topk(Q, I, k)
    if metric in ("cosine", "correlation", "hellinger"):
        Q, I = metric_rows(Q, metric), metric_rows(I, metric)
    elif metric not in TILE_METRICS and metric != "sqeuclidean":
        raise ValueError(f"unknown metric {metric!r}")
    nq, ni, d = Q.shape[0], I.shape[0], I.shape[1]
    k = min(k, ni)
    per_pair = max(1, d) if metric in TILE_METRICS else 1
    ichunk = max(k, min(ni, 4096))
    qchunk = max(1, block_elems // (ichunk * per_pair))
    dists = torch.empty((nq, k), dtype=torch.float32, device=Q.device)
    idx = torch.empty((nq, k), dtype=torch.int64, device=Q.device)
    for s in range(0, nq, qchunk):
        e = min(nq, s + qchunk)
        best_d = best_i = None
        for s2 in range(0, ni, ichunk):
            e2 = min(ni, s2 + ichunk)
            keys = _metric_keys(Q[s:e], I[s2:e2], metric, p, block_elems)
            vals, ids = torch.topk(keys, min(k, e2 - s2), dim=1, largest=False)
            ids = ids + s2
            if best_d is not None:
                vals = torch.cat([best_d, vals], dim=1)
                ids = torch.cat([best_i, ids], dim=1)
                vals, order = torch.topk(vals, min(k, vals.shape[1]), dim=1, largest=False)
                ids = ids.gather(1, order)
            best_d, best_i = vals, ids
        best_d, order = torch.sort(best_d, dim=1)
        dists[s:e] = finish_keys(best_d, metric, p, d)
        idx[s:e] = best_i.gather(1, order)
    return dists, idx


# metrics defined for sparse (CSR) input: every one has f(0, 0) = 0 and sums
# over coordinates, so a pair's distance needs only the stored entries.
# chebyshev (a max) and correlation (centring fills the row) do not qualify.
SPARSE_METRICS = (
    "euclidean", "sqeuclidean", "cosine", "hellinger",
    "manhattan", "minkowski", "canberra", "hamming", "jaccard",
)


def _jaccard_keys(Q: torch.Tensor, I: torch.Tensor) -> torch.Tensor:
    """[q, n] jaccard distances of the boolean (nonzero) patterns of dense
    rows; two empty rows are at distance 0."""
    Qb = (Q != 0).to(torch.float32)
    Ib = (I != 0).to(torch.float32)
    inter = Qb @ Ib.T
    union = Qb.sum(dim=1)[:, None] + Ib.sum(dim=1)[None, :] - inter
    return torch.where(union > 0, 1.0 - inter / union.clamp(min=1.0), torch.zeros_like(inter))


def knn_topk_metric_sparse(
    Q: Any,
    I: Any,
    k: int,
    metric: str = "euclidean",
    p: float = 2.0,
    device: Any = None,
    block_elems: int = 1 << 24,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Brute-force kNN of scipy CSR queries against scipy CSR items under a
    canonical metric of SPARSE_METRICS: (dists f32 [q,k] ascending, idx int64
    [q,k]) on `device`. Row chunks of both sides are densified, never more
    than block_elems elements at a time, and go through `_metric_keys`;
    jaccard is computed from the boolean rows."""
    if metric not in SPARSE_METRICS:
        raise ValueError(f"metric {metric!r} is not supported for sparse input")
    dev = torch.device(device) if device is not None else torch.device("cpu")
    nq, ni, d = Q.shape[0], I.shape[0], I.shape[1]
    k = min(k, ni)
    key_metric = "sqeuclidean" if metric == "euclidean" else metric

    def dense(M, s, e):
        X = torch.from_numpy(M[s:e].toarray().astype("float32", copy=False)).to(dev)
        if metric in ("cosine", "hellinger"):
            X = metric_rows(X, metric)
        return X

    ichunk = max(k, min(ni, 4096, max(1, block_elems // max(1, d))))
    qchunk = max(1, min(nq, block_elems // max(1, d, ichunk)))
    dists = torch.empty((nq, k), dtype=torch.float32, device=dev)
    idx = torch.empty((nq, k), dtype=torch.int64, device=dev)
    for s in range(0, nq, qchunk):
        e = min(nq, s + qchunk)
        Qd = dense(Q, s, e)
        best_d = best_i = None
        for s2 in range(0, ni, ichunk):
            e2 = min(ni, s2 + ichunk)
            Id = dense(I, s2, e2)
            if metric == "jaccard":
                keys = _jaccard_keys(Qd, Id)
            else:
                keys = _metric_keys(Qd, Id, key_metric, p, block_elems)
            vals, ids = torch.topk(keys, min(k, e2 - s2), dim=1, largest=False)
            ids = ids + s2
            if best_d is not None:
                vals = torch.cat([best_d, vals], dim=1)
                ids = torch.cat([best_i, ids], dim=1)
                vals, order = torch.topk(vals, min(k, vals.shape[1]), dim=1, largest=False)
                ids = ids.gather(1, order)
            best_d, best_i = vals, ids
        best_d, order = torch.sort(best_d, dim=1)
        out = finish_keys(best_d, key_metric, p, d)
        dists[s:e] = torch.sqrt(out) if metric == "euclidean" else out
        idx[s:e] = best_i.gather(1, order)
    return dists, idx


def softmax_residual(
    scores: torch.Tensor, y_idx: torch.Tensor
) -> Tuple[torch.Tensor, torch.Tensor]:
    """(resid [n,C], loss sum) — sigmoid when C==1 else softmax."""
    n, C = scores.shape[0], scores.shape[1] if scores.dim() > 1 else 1
    if C == 1:
        z = scores[:, 0]
        t = y_idx.to(z.dtype) * 2.0 - 1.0
        loss = torch.nn.functional.softplus(-t * z).sum()
        resid = (torch.sigmoid(z) - y_idx.to(z.dtype))[:, None]
    else:
        logp = torch.log_softmax(scores, dim=1)
        loss = -logp.gather(1, y_idx.view(-1, 1).to(torch.int64)).sum()
        resid = torch.exp(logp)
        resid.scatter_add_(
            1,
            y_idx.view(-1, 1).to(torch.int64),
            -torch.ones_like(y_idx, dtype=resid.dtype).view(-1, 1),
        )
    return resid, loss.reshape(())


def logistic_forward_grad(
    X: torch.Tensor,
    y_idx: torch.Tensor,
    W: torch.Tensor,
    fit_intercept: bool,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """One multinomial/binary logistic pass on the local shard.

    W is [C, d(+1)] with the intercept LAST column when fit_intercept.
    Binary (C==1): sigmoid/binomial loss in Spark's parametrization.
    Returns (grad [C, d(+1)] UNSCALED sum over local rows, loss scalar sum).
    """
    n, d = X.shape
    C = W.shape[0]
    coef = W[:, :d]
    scores = X @ coef.T
    if fit_intercept:
        scores = scores + W[:, d][None, :]
    if C == 1:
        z = scores[:, 0]
        # log(1+exp(-t*z)) with t in {-1,1}; y_idx in {0,1}
        t = y_idx.to(z.dtype) * 2.0 - 1.0
        loss = torch.nn.functional.softplus(-t * z).sum()
        p = torch.sigmoid(z)
        resid = (p - y_idx.to(z.dtype))[:, None]  # [n,1]
    else:
        logp = torch.log_softmax(scores, dim=1)
        loss = -logp.gather(1, y_idx.view(-1, 1).to(torch.int64)).sum()
        p = torch.exp(logp)
        p.scatter_add_(
            1,
            y_idx.view(-1, 1).to(torch.int64),
            -torch.ones_like(y_idx, dtype=p.dtype).view(-1, 1),
        )
        resid = p  # [n,C] = softmax - onehot
    grad_coef = resid.T @ X  # [C,d]
    if fit_intercept:
        grad = torch.cat([grad_coef, resid.sum(dim=0)[:, None]], dim=1)
    else:
        grad = grad_coef
    return grad, loss.reshape(())
