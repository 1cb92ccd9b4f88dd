"""k-NN ops: fused MFMA distance + in-LDS top-k selection.

HIP path (gfx950): `knn_select` streams 128-item tiles against 64-query
blocks, fusing the ||q-i||^2 expansion (MFMA) with per-query top-k candidate
pools held in LDS — the [nq, ni] distance matrix is never materialized
(reference NearestNeighborsMG tiled distance + top-k).
Falls back to the chunked torch path for k > 64 or CPU.

`knn_topk_metric` serves the metrics other than euclidean (UMAP's `metric`):
dot-product metrics on preprocessed rows through the same GEMM + selection
path, per-coordinate metrics through the `pairwise_dist` tile kernel +
`knn_merge_topk_keys`. `knn_topk_metric_sparse` is its CSR twin: the
`csr_pairwise` kernel walks only the stored entries of both sides.
"""

from __future__ import annotations

import math
from typing import Any, Callable, Dict, Tuple

import numpy as np
import torch

from . import torch_ref
from .dispatch import hip_ops, use_hip


def knn_topk(Q: torch.Tensor, I: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(dists [q,k] euclidean, idx int64 [q,k]) of queries against items.

    Default GPU path: hipBLASLt GEMM for the dot block + the OWN
    `knn_merge_topk` kernel, which fuses the ||q-i||^2 expansion with a
    running per-query top-k — the [q, chunk] distance matrix is never
    materialized and each GEMM output byte is read exactly once (the old
    torch path wrote d2, re-read it with multi-pass torch.topk and merged
    chunks with cat+topk+gather). SRML_KNN_KERNEL=1 keeps the all-in-one
    MFMA knn_select kernel (measured slower at 1M items; profiles/README.md),
    SRML_KNN_KERNEL=0 forces the torch reference path."""
    import os

    mode = os.environ.get("SRML_KNN_KERNEL", "")
    k_eff = min(k, I.shape[0])
    if mode == "1" and use_hip(Q, I) and k_eff <= 64 and Q.dtype == torch.float32:
        ext = hip_ops()
        d2, idx = ext.knn_select(Q.contiguous(), I.contiguous(), k_eff)
        return torch.sqrt(torch.clamp(d2, min=0.0)), idx
    if (
        mode != "0"
        and use_hip(Q, I)
        and k_eff == k
        and k <= 64
        and Q.dtype == torch.float32
        and I.dtype == torch.float32
        and Q.shape[0] > 0
    ):
        return _knn_topk_gemm_select(Q.contiguous(), I.contiguous(), k)
    return torch_ref.knn_topk(Q, I, k)


def _chunked_select(
    nq: int,
    ni: int,
    k: int,
    dev: torch.device,
    chunk_elems: int,
    merge_chunk: Callable[[torch.Tensor, int, int, torch.Tensor, torch.Tensor], None],
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Running 64-slot top-k over item chunks: `merge_chunk(Gv, s, e, best_d,
    best_i)` fills the [nq, e-s] scratch block Gv for items s:e and merges it
    into the slots. Returns the k smallest keys per row, ascending, and their
    item indices."""
    # 64 candidate slots per query; lanes >= k carry a -inf sentinel so they
    # never own tau (the running worst kept distance) inside the kernel
    best_d = torch.full((nq, 64), float("inf"), dtype=torch.float32, device=dev)
    if k < 64:
        best_d[:, k:] = float("-inf")
    best_i = torch.full((nq, 64), -1, dtype=torch.int64, device=dev)

    # multiple of 64 so every non-final chunk keeps the kernel's float4 path
    # (row base 16B-aligned requires chunk width % 4 == 0)
    ichunk = max(256, (min(ni, chunk_elems // max(1, nq)) // 64) * 64)
    G = torch.empty((nq, min(ichunk, ni)), dtype=torch.float32, device=dev)
    for s in range(0, ni, ichunk):
        e = min(ni, s + ichunk)
        # the kernel wants a contiguous [nq, e-s] block (row stride == e-s)
        Gv = G if e - s == G.shape[1] else torch.empty(
            (nq, e - s), dtype=torch.float32, device=dev
        )
        merge_chunk(Gv, s, e, best_d, best_i)

    if k < 64:
        best_d[:, k:] = float("inf")  # dead slots sort last
    d_sorted, order = torch.sort(best_d, dim=1)
    i_sorted = best_i.gather(1, order)
    return d_sorted[:, :k], i_sorted[:, :k].contiguous()


def _gemm_select_keys(
    Q: torch.Tensor,
    I: torch.Tensor,
    q_sq: torch.Tensor,
    i_sq: torch.Tensor,
    k: int,
    chunk_elems: int,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """k smallest q_sq[r] + i_sq[j] - 2 <Q[r], I[j]> per row: library GEMM for
    the dot block + the own `knn_merge_topk` selection kernel."""
    ext = hip_ops()

    def merge_chunk(Gv, s, e, best_d, best_i):
        torch.mm(Q, I[s:e].T, out=Gv)
        ext.knn_merge_topk(Gv, q_sq, i_sq[s:e].contiguous(), s, best_d, best_i)

    return _chunked_select(Q.shape[0], I.shape[0], k, Q.device, chunk_elems, merge_chunk)


def _knn_topk_gemm_select(
    Q: torch.Tensor, I: torch.Tensor, k: int, chunk_elems: int = 1 << 29
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Library GEMM + own running-top-k selection kernel (see knn_topk)."""
    q_sq = (Q * Q).sum(dim=1).contiguous()
    i_sq = (I * I).sum(dim=1).contiguous()
    d2, idx = _gemm_select_keys(Q, I, q_sq, i_sq, k, chunk_elems)
    return torch.sqrt(torch.clamp(d2, min=0.0)), idx


# ---------------------------------------------------------------------------
# metrics other than euclidean (UMAP's `metric`; scipy cdist definitions)
# ---------------------------------------------------------------------------

# alias -> canonical name
METRIC_ALIASES: Dict[str, str] = {
    "euclidean": "euclidean", "l2": "euclidean",
    "sqeuclidean": "sqeuclidean",
    "cosine": "cosine",
    "correlation": "correlation",
    "hellinger": "hellinger",
    "manhattan": "manhattan", "l1": "manhattan", "cityblock": "manhattan",
    "taxicab": "manhattan",
    "chebyshev": "chebyshev", "linf": "chebyshev",
    "minkowski": "minkowski",
    "canberra": "canberra",
    "hamming": "hamming",
}
# per-coordinate reductions served by the `pairwise_dist` kernel -> its op code
TILE_OPS: Dict[str, int] = {
    "manhattan": 0, "chebyshev": 1, "minkowski": 2, "canberra": 3, "hamming": 4,
}


def resolve_metric(metric: str, p: float = 2.0, sparse: bool = False) -> Tuple[str, float]:
    """(canonical metric, p) of a metric name or alias. minkowski with p = 1
    and p = 2 resolves to manhattan and euclidean. ValueError for jaccard
    (dense inputs), an unknown name, or a p that is not finite and > 0.
    With `sparse`, jaccard resolves and the metrics that have no sparse form
    (chebyshev, correlation) raise ValueError."""
    name = str(metric).lower()
    if name == "jaccard":
        if sparse:
            return "jaccard", 2.0
        raise ValueError("Metric 'jaccard' not supported for dense inputs.")
    if sparse and METRIC_ALIASES.get(name) in ("chebyshev", "correlation"):
        raise ValueError(
            f"metric {METRIC_ALIASES[name]!r} is not supported for sparse input "
            f"(accepted: {', '.join(torch_ref.SPARSE_METRICS)})"
        )
    if name not in METRIC_ALIASES:
        raise ValueError(
            f"Unknown metric {metric!r}; accepted: {', '.join(sorted(METRIC_ALIASES))}"
        )
    name = METRIC_ALIASES[name]
    if name != "minkowski":
        return name, 2.0
    p = float(p)
    if not (math.isfinite(p) and p > 0):
        raise ValueError(f"minkowski p must be finite and > 0, got {p!r}")
    if p == 1.0:
        return "manhattan", 2.0
    if p == 2.0:
        return "euclidean", 2.0
    return name, p


def knn_topk_metric(
    Q: torch.Tensor,
    I: torch.Tensor,
    k: int,
    metric: str = "euclidean",
    p: float = 2.0,
    chunk_elems: int = 1 << 29,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """(dists f32 [q,k] ascending, idx int64 [q,k]) of queries against items
    under `metric` (any name of METRIC_ALIASES; `p` for minkowski).

    euclidean is `knn_topk`, verbatim. On the GPU the GEMM family (sqeuclidean,
    cosine, correlation, hellinger) preprocesses the rows in torch and reuses
    library GEMM + `knn_merge_topk`; the tile family (manhattan, chebyshev,
    minkowski, canberra, hamming) runs the `pairwise_dist` kernel per item
    chunk + `knn_merge_topk_keys`, the root / division by d applied to the k
    survivors only. CPU tensors, k > 64 and non-f32 input take the chunked
    torch path."""
    metric, p = resolve_metric(metric, p)
    if metric == "euclidean":
        return knn_topk(Q, I, k)
    kernel_path = (
        use_hip(Q, I)
        and k <= min(64, I.shape[0])
        and Q.dtype == torch.float32
        and I.dtype == torch.float32
        and Q.shape[0] > 0
    )
    if not kernel_path:
        return torch_ref.knn_topk_metric(Q, I, k, metric, p)
    if metric in TILE_OPS:
        keys, idx = _tile_select_keys(
            Q.contiguous(), I.contiguous(), k, TILE_OPS[metric], p, chunk_elems
        )
    elif metric == "sqeuclidean":
        Q, I = Q.contiguous(), I.contiguous()
        q_sq = (Q * Q).sum(dim=1).contiguous()
        i_sq = (I * I).sum(dim=1).contiguous()
        keys, idx = _gemm_select_keys(Q, I, q_sq, i_sq, k, chunk_elems)
    else:
        # key = 1 - <q', i'>: q_sq = 1, i_sq = 0 and the query rows halved
        # (exact) so that knn_merge_topk's -2*dot is -<q', i'>
        Qp = (torch_ref.metric_rows(Q, metric) * 0.5).contiguous()
        Ip = torch_ref.metric_rows(I, metric).contiguous()
        q_sq = torch.ones(Q.shape[0], dtype=torch.float32, device=Q.device)
        i_sq = torch.zeros(I.shape[0], dtype=torch.float32, device=Q.device)
        keys, idx = _gemm_select_keys(Qp, Ip, q_sq, i_sq, k, chunk_elems)
    return torch_ref.finish_keys(keys, metric, p, I.shape[1]), idx


def _tile_select_keys(
    Q: torch.Tensor, I: torch.Tensor, k: int, op: int, p: float, chunk_elems: int
) -> Tuple[torch.Tensor, torch.Tensor]:
    """k smallest `pairwise_dist` keys per row, chunked as the GEMM path is."""
    ext = hip_ops()

    def merge_chunk(Gv, s, e, best_d, best_i):
        ext.pairwise_dist(Q, I[s:e], op, float(p), Gv)
        ext.knn_merge_topk_keys(Gv, s, best_d, best_i)

    return _chunked_select(Q.shape[0], I.shape[0], k, Q.device, chunk_elems, merge_chunk)


# ---------------------------------------------------------------------------
# sparse (CSR) input: the `csr_pairwise` kernel in place of `pairwise_dist`
# ---------------------------------------------------------------------------

# metric -> `csr_pairwise` op code
SPARSE_OPS: Dict[str, int] = {
    "euclidean": 0, "sqeuclidean": 0, "cosine": 0, "hellinger": 0,
    "manhattan": 1, "minkowski": 2, "canberra": 3, "hamming": 4, "jaccard": 5,
}
# items per `csr_pairwise` call: 4 query rows x chunk f32 accumulators of LDS
# per block (8192 -> 128 KB, one block per CU; profiles/README.md)
SPARSE_CHUNK = 8192


def canonical_csr(M: Any) -> Any:
    """scipy CSR, f32, column ids sorted within a row, no stored zeros. The
    input is not modified."""
    import scipy.sparse as sp

    if not sp.issparse(M):
        M = sp.csr_matrix(np.asarray(M, dtype=np.float32))
    out = M.tocsr().astype(np.float32)  # astype copies
    out.sum_duplicates()
    out.eliminate_zeros()
    out.sort_indices()
    return out


def _sparse_rows(M: Any, metric: str, p: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(values, per-row constant) of a canonical CSR under `metric`, both f32
    host tensors: values preprocessed as the dense path preprocesses rows
    (unit rows for cosine, sqrt for hellinger), the constant sum_j f(x_j, 0).
    The row sums are taken on the host in one fixed order (a device
    index_add_ is atomic), which the bit-reproducible graph needs."""
    vals = M.data
    n = M.shape[0]
    counts = np.diff(M.indptr)
    filled = counts > 0

    def row_sum(v: np.ndarray) -> torch.Tensor:
        out = np.zeros(n, dtype=np.float32)
        if v.size:  # empty rows own no segment
            out[filled] = np.add.reduceat(v, M.indptr[:-1][filled])
        return torch.from_numpy(out)

    zeros = torch.zeros(n, dtype=torch.float32)
    if metric in ("euclidean", "sqeuclidean"):
        const = row_sum(vals * vals)
    elif metric == "cosine":
        norm = np.sqrt(row_sum(vals * vals).numpy())
        if bool((norm == 0).any()):
            raise ValueError("metric='cosine' is undefined for zero-norm rows")
        vals, const = vals / np.repeat(norm, counts), zeros
    elif metric == "hellinger":
        if bool((vals < 0).any()):
            raise ValueError("metric='hellinger' requires non-negative inputs")
        vals, const = np.sqrt(vals), zeros
    elif metric == "manhattan":
        const = row_sum(np.abs(vals))
    elif metric == "minkowski":
        const = row_sum(np.abs(vals) ** np.float32(p))
    else:  # canberra, hamming, jaccard: nnz
        const = torch.from_numpy(counts.astype(np.float32))
    return torch.from_numpy(vals), const


def knn_topk_metric_sparse(
    Q: Any,
    I: Any,
    k: int,
    metric: str = "euclidean",
    p: float = 2.0,
    device: Any = None,
    chunk: int = SPARSE_CHUNK,
    chunk_elems: int = 1 << 29,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """(dists f32 [q,k] ascending, idx int64 [q,k]) of scipy CSR queries
    against scipy CSR items under `metric`, on `device` (default: the GPU
    where there is one). Accepted: euclidean/l2, sqeuclidean, cosine,
    hellinger, manhattan and its aliases, minkowski, canberra, hamming,
    jaccard; chebyshev and correlation raise ValueError.

    On the GPU each item chunk is turned into CSC in torch and the
    `csr_pairwise` kernel writes its [q, chunk] key block, which
    `knn_merge_topk_keys` folds into the running top-k; only stored entries
    are ever touched. The block never exceeds `chunk_elems` elements (2 GB by
    default, as on the dense path): queries are taken in tiles of
    chunk_elems // chunk rows, each against every item chunk. CPU devices
    and k > 64 take the torch path, which densifies bounded row chunks."""
    metric, p = resolve_metric(metric, p, sparse=True)
    if Q.shape[1] != I.shape[1]:
        raise ValueError(f"queries have {Q.shape[1]} columns, items {I.shape[1]}")
    same = Q is I
    I = canonical_csr(I)
    Q = I if same else canonical_csr(Q)
    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    dev = torch.device(device)
    nq, ni, d = Q.shape[0], I.shape[0], I.shape[1]
    kernel_path = (
        dev.type == "cuda"
        and use_hip(torch.empty(0, device=dev))
        and k <= min(64, ni)
        and nq > 0
    )
    if not kernel_path:
        return torch_ref.knn_topk_metric_sparse(Q, I, k, metric, p, dev)
    if d >= 1 << 31:
        raise ValueError("sparse kNN supports fewer than 2^31 columns")
    if not 256 <= chunk <= SPARSE_CHUNK:  # 256: _chunked_select's floor
        raise ValueError(f"chunk must be in [256, {SPARSE_CHUNK}]")
    ext = hip_ops()
    op = SPARSE_OPS[metric]

    i_val, B = _sparse_rows(I, metric, p)
    q_val, A = (i_val, B) if same else _sparse_rows(Q, metric, p)
    if metric in ("cosine", "hellinger"):
        # key = 1 - <q', x'>: A = 1, B = 0 and the query values halved (exact)
        # so that the kernel's -2 acc is -<q', x'>, as in knn_topk_metric
        q_val = q_val * 0.5
        A = torch.ones(nq, dtype=torch.float32)
    q_ptr = torch.from_numpy(Q.indptr.astype(np.int64)).to(dev)
    q_col = torch.from_numpy(Q.indices.astype(np.int32)).to(dev)
    q_val = q_val.contiguous().to(dev)
    A = A.to(dev)
    B = B.to(dev)
    i_ptr = I.indptr.astype(np.int64)  # host: chunk bounds cost no sync
    i_col = torch.from_numpy(I.indices.astype(np.int64)).to(dev)
    i_val = i_val.contiguous().to(dev)
    i_cnt = torch.from_numpy(np.diff(i_ptr)).to(dev)
    zero = torch.zeros(1, dtype=torch.int64, device=dev)

    def csc_chunk(s, e):
        a, b = int(i_ptr[s]), int(i_ptr[e])
        # CSC of item rows s:e: a stable sort by column id keeps the rows of
        # one column ascending
        cols, order = torch.sort(i_col[a:b], stable=True)
        local = torch.repeat_interleave(
            torch.arange(e - s, device=dev, dtype=torch.int32), i_cnt[s:e], output_size=b - a
        )
        colptr = torch.cat([zero, torch.cumsum(torch.bincount(cols, minlength=d), dim=0)])
        return colptr, local[order].contiguous(), i_val[a:b][order].contiguous()

    def select_tile(qs, qe):
        # indptr keeps its absolute offsets into q_col / q_val
        t_ptr, t_A = q_ptr[qs:qe + 1].contiguous(), A[qs:qe].contiguous()

        def merge_chunk(Gv, s, e, best_d, best_i):
            colptr, c_row, c_val = csc_chunk(s, e)
            ext.csr_pairwise(
                t_ptr, q_col, q_val, colptr, c_row, c_val, t_A, B[s:e].contiguous(),
                op, float(p), Gv,
            )
            ext.knn_merge_topk_keys(Gv, s, best_d, best_i)

        return _chunked_select(qe - qs, ni, k, dev, chunk * (qe - qs), merge_chunk)

    # one tile unless nq * chunk passes the budget (65 536 rows at 8192 items);
    # beyond it each tile rebuilds the chunk CSCs, a sort of nnz per tile
    qtile = max(4, chunk_elems // chunk)
    tiles = [select_tile(qs, min(nq, qs + qtile)) for qs in range(0, nq, qtile)]
    keys = torch.cat([t[0] for t in tiles]) if len(tiles) > 1 else tiles[0][0]
    idx = torch.cat([t[1] for t in tiles]) if len(tiles) > 1 else tiles[0][1]
    if metric == "euclidean":
        return torch.sqrt(torch.clamp(keys, min=0.0)), idx
    return torch_ref.finish_keys(keys, metric, p, d), idx
