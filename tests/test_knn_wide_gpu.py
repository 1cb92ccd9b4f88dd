"""`knn_merge_topk_wide` (64 < k <= 1024) against exact integer references.

Inputs are small integers held in f32, as in test_hip_ops_exact.py: every d2
and every key is an integer below 2**24 in any summation order, so the kernel
must return exactly the reference's k smallest. Every check is tie-invariant.
"""

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from spark_rapids_ml_amd.ops import knn as knn_ops
from spark_rapids_ml_amd.ops import torch_ref

pytestmark = pytest.mark.gpu
LIM = 2 ** 24


@pytest.fixture(scope="module")
def ext():
    from spark_rapids_ml_amd.ops.dispatch import hip_ops

    return hip_ops()


def _case(nq, ni, d, order=None):
    """(Q, I, D): integer rows in [-8, 8] and their int64 squared distances;
    `order` sorts the items by distance to query 0 ("asc" / "desc")."""
    assert 4 * 64 * d < LIM  # (q-i)^2 <= 256 per coordinate, so is every partial sum
    rng = np.random.default_rng(100 * ni + d)
    Q = rng.integers(-8, 9, size=(nq, d)).astype(np.float64)
    I = rng.integers(-8, 9, size=(ni, d)).astype(np.float64)
    dist = lambda: ((Q * Q).sum(1)[:, None] + (I * I).sum(1)[None, :] - 2.0 * (Q @ I.T)).astype(np.int64)
    if order:
        I = I[np.argsort(dist()[0] * (1 if order == "asc" else -1), kind="stable")]
    return Q, I, dist()


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _check(keys, ids, D, k, rel=0.0):
    """keys ascending; ids unique and in range; the keys named by the ids are
    the reference's k smallest; each returned key is (within rel of) D[row, id]."""
    keys, ids = keys.cpu().numpy().astype(np.float64), ids.cpu().numpy()
    assert keys.shape == ids.shape == (D.shape[0], k)
    assert ids.min() >= 0 and ids.max() < D.shape[1]
    assert all(len(set(r)) == k for r in ids.tolist())
    named = np.take_along_axis(D, ids, axis=1).astype(np.float64)
    assert np.array_equal(np.sort(named, axis=1), np.sort(D, axis=1)[:, :k])
    assert (np.diff(keys, axis=1) >= 0).all()
    want = np.sqrt(named) if rel else named
    assert (np.abs(keys - want) <= rel * want).all()


KERNEL_CASES = [
    # nq, ni, d, k, chunk width, item order
    (1, 65, 4, 65, 65, None),         # smallest wide call, ni == k, 63 dead positions
    (5, 300, 8, 128, 300, None),      # k == K
    (5, 300, 8, 129, 300, None),      # one past: K = 256
    (5, 1300, 8, 1024, 1300, None),   # the cap
    (5, 2051, 8, 1024, 256, None),    # nine calls, list fills in the fourth, last 3 wide
    (1, 1999, 8, 256, 1999, "desc"),  # every column passes tau
    (1, 1999, 8, 256, 1999, "asc"),   # nothing enters after the first k
]


@pytest.mark.parametrize("nq,ni,d,k,width,order", KERNEL_CASES)
def test_merge_topk_wide(ext, nq, ni, d, k, width, order):
    Q, I, D = _case(nq, ni, d, order)
    Qt, It = _f32(Q), _f32(I)
    q_sq, i_sq = (Qt * Qt).sum(1), (It * It).sum(1)
    state = torch.full((nq, knn_ops._wide_slots(k)), -1, dtype=torch.int64, device="cuda")
    for s in range(0, ni, width):
        G = (Qt @ It[s:s + width].T).contiguous()
        ext.knn_merge_topk_wide(G, q_sq, i_sq[s:s + width].contiguous(), s, state, k)
    _check(*knn_ops._wide_unpack(state, k), D, k)


def test_merge_topk_wide_keys_negative_and_tied(ext):
    nq, ni, k = 5, 700, 100
    rng = np.random.default_rng(7)
    D = rng.integers(-500, 501, size=(nq, ni))  # ~1000 values over 700 columns: ties
    D[:, ::7] = 0
    D[0, :300] = -500  # a tie across the k-th position
    Kf = D.astype(np.float32)
    Kf[(D == 0) & (np.arange(ni) % 14 == 0)] = -0.0
    state = torch.full((nq, 128), -1, dtype=torch.int64, device="cuda")
    for s in range(0, ni, 256):
        ext.knn_merge_topk_wide_keys(_f32(Kf[:, s:s + 256]), s, state, k)
    keys, ids = knn_ops._wide_unpack(state, k)
    _check(keys, ids, D, k)
    # smallest id wins a tie: row 0 is the first 100 of its 300 equal keys
    assert ids[0].cpu().tolist() == list(range(100))


@pytest.mark.parametrize("family", ["euclidean", "manhattan", "jaccard"])
def test_dispatch_reaches_wide_kernel(monkeypatch, family):
    def no_fallback(*a, **kw):
        raise AssertionError("k = 100 fell back to the torch path")

    for name in ("knn_topk", "knn_topk_metric", "knn_topk_metric_sparse"):
        monkeypatch.setattr(torch_ref, name, no_fallback)
    nq, ni, k = 9, 700, 100
    Q, I, D = _case(nq, ni, 8)
    if family == "euclidean":
        keys, ids = knn_ops._knn_topk_gemm_select(_f32(Q), _f32(I), k, chunk_elems=256 * nq)
        assert knn_ops.knn_topk(_f32(Q), _f32(I), k)[1].shape == (nq, k)  # the gate itself
        _check(keys, ids, D, k, rel=4.8e-7)  # 4 ulp of f32 for the one rounding of the root
    elif family == "manhattan":
        D = np.abs(Q[:, None, :] - I[None, :, :]).sum(2).astype(np.int64)
        keys, ids = knn_ops.knn_topk_metric(_f32(Q), _f32(I), k, "manhattan", chunk_elems=256 * nq)
        _check(keys, ids, D, k)
    else:
        rng = np.random.default_rng(3)
        Qb, Ib = rng.random((nq, 40)) < 0.3, rng.random((ni, 40)) < 0.3
        inter = Qb.astype(np.int64) @ Ib.astype(np.int64).T
        union = Qb.sum(1)[:, None] + Ib.sum(1)[None, :] - inter
        # a ratio of integers < 2**11: its f64 value rounds to f32 as the exact one does
        D = np.where(union > 0, (union - inter) / np.maximum(union, 1), 0.0).astype(np.float32)
        keys, ids = knn_ops.knn_topk_metric_sparse(
            sp.csr_matrix(Qb.astype(np.float32)), sp.csr_matrix(Ib.astype(np.float32)), k,
            "jaccard", device="cuda", chunk=256, chunk_elems=256 * 4,
        )
        _check(keys, ids, D.astype(np.float64), k)


def test_public_models_at_k_100(monkeypatch):
    from spark_rapids_ml_amd import UMAP, NearestNeighbors
    from spark_rapids_ml_amd.data import DataFrame

    def no_fallback(*a, **kw):
        raise AssertionError("k > 64 fell back to the torch path")

    monkeypatch.setattr(torch_ref, "knn_topk", no_fallback)
    _, X, _ = _case(1, 600, 8)
    X = X.astype(np.float32)
    D = ((X[:, None, :] - X[None, :, :]) ** 2).sum(2).astype(np.int64)
    df = DataFrame.from_numpy(X)
    _, _, knn = NearestNeighbors(k=100).fit(df).kneighbors(df)
    _check(torch.from_numpy(np.asarray(knn["distances"], dtype=np.float32)),
           torch.from_numpy(np.asarray(knn["indices"], dtype=np.int64)), D, 100, rel=4.8e-7)
    emb = UMAP(n_neighbors=100, n_epochs=20, random_state=1).fit(
        DataFrame.from_numpy(X[:400, :6])).embedding
    assert emb.shape == (400, 2) and np.isfinite(emb).all()


def test_limits(ext):
    Q, I, D = _case(3, 1100, 8)
    keys, ids = knn_ops.knn_topk(_f32(Q), _f32(I), 1025)  # past the cap: torch path
    _check(keys, ids, D, 1025, rel=4.8e-7)
    G = torch.zeros((3, 300), device="cuda")
    for k, width in ((64, 128), (1025, 2048), (100, 256)):
        with pytest.raises(RuntimeError):
            ext.knn_merge_topk_wide_keys(
                G, 0, torch.full((3, width), -1, dtype=torch.int64, device="cuda"), k)
