"""The `csr_pairwise` HIP kernel alone, against f64 keys of the densified rows.

Values are integers in {1..4}, so every intermediate of the dot, L1, hamming
and jaccard ops is an exact f32 integer (jaccard ends in one correctly rounded
quotient of two of them): those are compared BIT-EQUAL to the f64 key rounded
to f32. Two ops cannot be exact:

canberra  each term |v-w|/(|v|+|w|) - 2 is a rounded quotient. Bound, absolute:
          gamma_{2m+8} * 4m, m the largest row nnz (at most 2m terms of
          magnitude <= 2 summed with A + B <= 2m; 8 roundings of slack for the
          quotient and the final sums), gamma_n = nU / (1 - nU), U = 2^-24.
Lp        |.|^p is exp2(p * log2|.|) on the transcendental unit (1 ulp each),
          so 3^3 is not 27 to the bit. Per power the relative error is
          (ln2 * 3 * p * log2(4) + 2) U <= 14.5 U for p = 3 (the derivation of
          tests/test_pairwise_metrics.py::_lp_bound with integer inputs, whose
          differences are exact); at most 2m + 2 such values of total
          magnitude <= 2 (A + B) are summed: 2 gamma_{2m+14} (A + B), absolute.

Shapes are the smallest that reach each path: nq not a multiple of the 4 rows
of a block, c on both sides of one and of several 64-lane strides, a column
list longer than 64, a single-entry column, an empty column, empty rows on both
sides, a column id past 2^16, and two item chunks through
`knn_topk_metric_sparse`.
"""

from functools import lru_cache

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from spark_rapids_ml_amd.ops import knn as knn_ops
from spark_rapids_ml_amd.ops.dispatch import hip_ops

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
DOT, L1, LP, CANBERRA, HAMMING, JACCARD = range(6)
OPS = [DOT, L1, LP, CANBERRA, HAMMING, JACCARD]
P = 3.0


def _gamma(n):
    return n * U / (1.0 - n * U)


@lru_cache(maxsize=None)
def _case(nq, c, d=40, density=0.3):
    """(Q csr [nq, d], I csr [c, d]) with values in {1..4}.

    Column 0 is held by every item but the empty one (a list longer than 64
    once c > 65) and by every non-empty query; column 1 by item 0 alone;
    column 2 by nobody. The last query row and the last item row are empty
    where there is more than one row; column d - 1 is stored on both sides."""
    rng = np.random.default_rng(1000 * nq + c + d)

    def side(n):
        M = (rng.random((n, min(d, 40))) < density) * rng.integers(1, 5, (n, min(d, 40)))
        M = M.astype(np.float32)
        M[:, 0] = rng.integers(1, 5, n)
        M[:, 1] = 0
        M[:, 2] = 0
        return M

    Qd, Id = side(nq), side(c)
    Id[0, 1] = 3.0
    Qd[0, 1] = 2.0
    last_q = np.array([1.0 + (r % 4) for r in range(nq)], dtype=np.float32)
    last_i = np.array([1.0 + (r % 3) for r in range(c)], dtype=np.float32)
    Q = sp.lil_matrix((nq, d), dtype=np.float32)
    I = sp.lil_matrix((c, d), dtype=np.float32)
    Q[:, : Qd.shape[1]] = Qd
    I[:, : Id.shape[1]] = Id
    Q[:, d - 1] = last_q[:, None]
    I[:, d - 1] = last_i[:, None]
    if nq > 1:
        Q[nq - 1, :] = 0
    if c > 1:
        I[c - 1, :] = 0
    Q, I = Q.tocsr(), I.tocsr()
    for M in (Q, I):
        M.eliminate_zeros()
        M.sort_indices()
    return Q, I


def _consts(M, op):
    v = M.data.astype(np.float64)
    if op == DOT:
        w = v * v
    elif op == L1:
        w = np.abs(v)
    elif op == LP:
        w = np.abs(v) ** P
    else:
        w = np.ones_like(v)
    rows = np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))
    return np.bincount(rows, weights=w, minlength=M.shape[0]).astype(np.float32)


def _run(Q, I, op):
    """The kernel's [nq, c] block for scipy CSR sides, CSC built by scipy."""
    dev = torch.device("cuda")
    C = I.tocsc()
    C.sort_indices()
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    out = torch.full((Q.shape[0], I.shape[0]), float("nan"), dtype=torch.float32, device=dev)
    hip_ops().csr_pairwise(
        t(Q.indptr, np.int64), t(Q.indices, np.int32), t(Q.data, np.float32),
        t(C.indptr, np.int64), t(C.indices, np.int32), t(C.data, np.float32),
        t(_consts(Q, op), np.float32), t(_consts(I, op), np.float32), op, P, out,
    )
    return out.cpu().numpy()


def _ref(Q, I, op):
    """f64 keys from the densified rows, one query row at a time."""
    Id = I.toarray().astype(np.float64)
    out = np.empty((Q.shape[0], I.shape[0]))
    for r in range(Q.shape[0]):
        q = Q[r].toarray().astype(np.float64)
        diff = np.abs(q - Id)
        if op == DOT:
            out[r] = (diff * diff).sum(1)
        elif op == L1:
            out[r] = diff.sum(1)
        elif op == LP:
            out[r] = (diff ** P).sum(1)
        elif op == CANBERRA:
            den = np.abs(q) + np.abs(Id)
            out[r] = np.where(den > 0, diff / np.where(den > 0, den, 1.0), 0.0).sum(1)
        elif op == HAMMING:
            out[r] = (q != Id).sum(1)
        else:
            inter = ((q != 0) & (Id != 0)).sum(1)
            union = ((q != 0) | (Id != 0)).sum(1)
            out[r] = np.where(union > 0, 1.0 - inter / np.maximum(union, 1), 0.0)
    return out


def _check(Q, I):
    m = int(max(np.diff(Q.indptr).max(), np.diff(I.indptr).max()))
    for op in OPS:
        got, want = _run(Q, I, op), _ref(Q, I, op)
        assert np.isfinite(got).all(), op
        if op == CANBERRA:
            err = np.abs(got - want).max()
            print(f"canberra max err {err:.3e}, bound {_gamma(2 * m + 8) * 4 * m:.3e}")
            assert err <= _gamma(2 * m + 8) * 4 * m
        elif op == LP:
            ab = _consts(Q, LP).astype(np.float64)[:, None] + _consts(I, LP).astype(np.float64)[None, :]
            bound = 2 * _gamma(2 * m + 14) * ab
            print(f"lp max err/bound {(np.abs(got - want) / np.maximum(bound, 1e-300)).max():.3e}")
            assert (np.abs(got - want) <= bound).all()
        else:
            assert np.array_equal(got, want.astype(np.float32)), op
        # the fixed accumulation order makes a second run bit-identical
        assert np.array_equal(got, _run(Q, I, op)), op


@pytest.mark.parametrize("c", [1, 63, 65, 257])
@pytest.mark.parametrize("nq", [1, 5, 9])
def test_keys_match_f64(nq, c):
    Q, I = _case(nq, c)
    if c > 65:
        assert np.diff(I.tocsc().indptr)[0] > 64  # several lane strides
    assert np.diff(I.tocsc().indptr)[1] == 1 and np.diff(I.tocsc().indptr)[2] == 0
    _check(Q, I)


def test_empty_rows_and_jaccard_of_two_empty_rows():
    Q, I = _case(5, 65)
    assert Q[4].nnz == 0 and I[64].nnz == 0
    got = _run(Q, I, JACCARD)
    assert got[4, 64] == 0.0  # two empty rows
    assert (got[4, :64] == 1.0).all() and (got[:4, 64] == 1.0).all()
    # an empty row's key is A + B
    l1 = _run(Q, I, L1)
    assert np.array_equal(l1[4], _consts(I, L1)) and np.array_equal(l1[:, 64], _consts(Q, L1))


def test_wide_column_ids():
    Q, I = _case(9, 65, d=70000)
    assert Q.indices.max() == 69999 and I.indices.max() == 69999
    _check(Q, I)


def test_two_chunks_through_knn_topk_metric_sparse(monkeypatch):
    """chunk + 1 items: the second chunk holds one item, a copy of query 0,
    which must come back as index `chunk` at distance 0."""
    from spark_rapids_ml_amd.ops import torch_ref

    def _no(*a, **k):
        raise AssertionError("torch fallback taken on the GPU")

    monkeypatch.setattr(torch_ref, "knn_topk_metric_sparse", _no)
    chunk, d, k = knn_ops.SPARSE_CHUNK, 50, 8
    rng = np.random.default_rng(5)
    Id = ((rng.random((chunk + 1, d)) < 0.2) * rng.integers(1, 5, (chunk + 1, d))).astype(np.float32)
    Qd = ((rng.random((5, d)) < 0.4) * rng.integers(1, 5, (5, d))).astype(np.float32)
    Id[chunk] = Qd[0]
    assert (np.abs(Id[:chunk] - Qd[0]).sum(1) > 0).all()
    dist, idx = knn_ops.knn_topk_metric_sparse(
        sp.csr_matrix(Qd), sp.csr_matrix(Id), k, "manhattan", device="cuda"
    )
    dist, idx = dist.cpu().numpy(), idx.cpu().numpy()
    full = np.abs(Qd[:, None, :].astype(np.float64) - Id[None, :, :]).sum(2)
    assert idx[0, 0] == chunk and dist[0, 0] == 0.0
    # integer distances tie: the k smallest VALUES are exact, and every index
    # returned lies at the distance returned for it
    assert np.array_equal(dist, np.sort(full, axis=1)[:, :k].astype(np.float32))
    assert np.array_equal(np.take_along_axis(full, idx, 1).astype(np.float32), dist)


def test_query_tiles_under_the_element_budget():
    """chunk_elems = 8 * 256 at 256-item chunks: 9 queries go in tiles of 8
    and 1, each against item chunks of 256 and 1; the result is the
    single-tile one to the bit."""
    Q, I = _case(9, 257)
    for metric in ("manhattan", "jaccard"):
        one = knn_ops.knn_topk_metric_sparse(Q, I, 8, metric, device="cuda")
        tiled = knn_ops.knn_topk_metric_sparse(
            Q, I, 8, metric, device="cuda", chunk=256, chunk_elems=8 * 256
        )
        # values to the bit; indices may differ among tied keys only
        assert torch.equal(one[0], tiled[0])
        full = _ref(Q, I, L1 if metric == "manhattan" else JACCARD)
        got = np.take_along_axis(full, tiled[1].cpu().numpy(), 1).astype(np.float32)
        assert np.array_equal(got, tiled[0].cpu().numpy())


def test_host_checks():
    Q, I = _case(5, 63)
    ext, dev = hip_ops(), torch.device("cuda")
    C = I.tocsc()
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    args = [
        t(Q.indptr, np.int64), t(Q.indices, np.int32), t(Q.data, np.float32),
        t(C.indptr, np.int64), t(C.indices, np.int32), t(C.data, np.float32),
        t(_consts(Q, L1), np.float32), t(_consts(I, L1), np.float32),
    ]
    out = torch.empty((5, 63), dtype=torch.float32, device=dev)
    with pytest.raises(RuntimeError, match="unknown csr_pairwise op"):
        ext.csr_pairwise(*args, 6, 2.0, out)
    with pytest.raises(RuntimeError, match=r"out must be \[nq, c\]"):
        ext.csr_pairwise(*args, L1, 2.0, out[:, :62].contiguous())
    with pytest.raises(RuntimeError, match="int32"):
        ext.csr_pairwise(*args[:1], args[1].to(torch.int64), *args[2:], L1, 2.0, out)
    with pytest.raises(RuntimeError, match="one device"):
        ext.csr_pairwise(*args[:7], args[7].cpu(), L1, 2.0, out)
    big = knn_ops.SPARSE_CHUNK + 1
    with pytest.raises(RuntimeError, match="limited to"):
        ext.csr_pairwise(
            *args[:7], torch.zeros(big, device=dev), L1, 2.0,
            torch.empty((5, big), dtype=torch.float32, device=dev),
        )
