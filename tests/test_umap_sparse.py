"""UMAP on sparse (CSR) input: the kNN graph stage against scipy on the
densified rows, the estimator's parameter rules, the CSR `rawData`, save ->
load -> transform and a two-rank fit.

The estimator runs on the process's device, so every unmarked test runs on
the CPU path where there is no GPU; the `gpu`-marked twins of the graph stage
additionally forbid the torch path (`kernel_only`).
"""

from functools import lru_cache

import numpy as np
import pytest
import scipy.sparse as sp
import torch
from scipy.spatial.distance import cdist

from spark_rapids_ml_amd import UMAP, UMAPModel
from spark_rapids_ml_amd.data import DataFrame
from spark_rapids_ml_amd.models import umap as umap_mod
from spark_rapids_ml_amd.ops import torch_ref

from .dist_utils import run_distributed

gpu = pytest.mark.gpu
U = 2.0 ** -24
N, D, K = 300, 2000, 15
GRAPH_METRICS = [
    "manhattan", "minkowski", "canberra", "sqeuclidean", "euclidean", "cosine",
    "hellinger", "hamming", "jaccard",
]


@pytest.fixture
def kernel_only(monkeypatch):
    def _no(*a, **k):
        raise AssertionError("torch fallback taken on the GPU")

    monkeypatch.setattr(torch_ref, "knn_topk_metric_sparse", _no)
    assert torch.cuda.is_available()


def _gamma(n):
    return n * U / (1.0 - n * U)


@lru_cache(maxsize=None)
def _data():
    """300 x 2000 CSR, 90-143 stored entries per row: ten sparse prototypes
    plus half of a sparse gamma(2, 1) noise matrix."""
    rng = np.random.default_rng(11)
    rvs = lambda n: rng.gamma(2.0, 1.0, n).astype(np.float32)
    M = sp.random(N, D, density=0.03, random_state=rng, data_rvs=rvs)
    proto = sp.random(10, D, density=0.03, random_state=rng, data_rvs=rvs).tocsr()
    lab = rng.integers(0, 10, N)
    X = (0.5 * M + proto[lab]).tocsr().astype(np.float32)
    X.eliminate_zeros()
    nnz = np.diff(X.indptr)
    assert (nnz.min(), nnz.max()) == (90, 143)
    return X


@lru_cache(maxsize=None)
def _metric_data(metric):
    """hellinger is a distance of distributions: rows scaled to sum to 1 (so
    the sqrt rows are unit rows and cosine's bound carries over)."""
    X = _data()
    if metric != "hellinger":
        return X
    s = np.asarray(X.sum(axis=1)).ravel().astype(np.float64)
    return sp.csr_matrix(sp.diags(1.0 / s) @ X.astype(np.float64)).astype(np.float32)


@lru_cache(maxsize=None)
def _graph_reference(metric):
    """(neighbour order [N, N-1] without self, their f64 keys, per-pair bound
    [N, N] on the f32 key). The key is the quantity the bound speaks of: the
    distance, its square for (sq)euclidean, its cube for minkowski p = 3.
    m is the largest row nnz:

      manhattan      2 gamma_{2m+6} (|q|_1 + |x|_1)
      minkowski p=3  2 gamma_{2m+14} (sum|q|^3 + sum|x|^3)
      canberra       gamma_{2m+8} 4m
      (sq)euclidean  2 gamma_{m+4} (|q|^2 + |x|^2)
      cosine         (m + 8) U
      hellinger      as cosine, on the sqrt rows
    """
    X = _metric_data(metric)
    Xd = X.toarray().astype(np.float64)
    m = int(np.diff(X.indptr).max())
    pair = lambda s: s[:, None] + s[None, :]
    if metric == "manhattan":
        key = cdist(Xd, Xd, "cityblock")
        bound = 2 * _gamma(2 * m + 6) * pair(np.abs(Xd).sum(1))
    elif metric == "minkowski":
        key = cdist(Xd, Xd, "minkowski", p=3) ** 3
        bound = 2 * _gamma(2 * m + 14) * pair((np.abs(Xd) ** 3).sum(1))
    elif metric == "canberra":
        key = cdist(Xd, Xd, "canberra")
        bound = np.full((N, N), _gamma(2 * m + 8) * 4 * m)
    elif metric in ("sqeuclidean", "euclidean"):
        key = cdist(Xd, Xd, "sqeuclidean")
        bound = 2 * _gamma(m + 4) * pair((Xd * Xd).sum(1))
    elif metric == "cosine":
        key = cdist(Xd, Xd, "cosine")
        bound = np.full((N, N), (m + 8) * U)
    elif metric == "hellinger":
        S = np.sqrt(Xd)
        key = 1.0 - S @ S.T
        bound = np.full((N, N), (m + 8) * U)
    elif metric == "hamming":
        key = cdist(Xd, Xd, "hamming")
        bound = None
    else:
        key = cdist(Xd != 0, Xd != 0, "jaccard")
        bound = None
    key = key.copy()
    np.fill_diagonal(key, np.inf)  # self excluded
    order = np.argsort(key, axis=1, kind="stable")[:, : N - 1]
    return order, np.take_along_axis(key, order, 1), bound


def _check_graph(knn_i, metric):
    """The rule of tests/test_umap_metrics.py::_check_graph. A row's set may
    differ from scipy's only where the reference's k-th and (k+1)-th keys are
    closer than twice the bound; at most 1 % of rows may. hamming and jaccard
    tie often: every strictly closer point is present and the rest lie exactly
    at the k-th distance (within 2U for jaccard, whose f32 value is a rounded
    quotient)."""
    order, key, bound = _graph_reference(metric)
    knn_i = np.asarray(knn_i)
    assert knn_i.shape == (N, K)
    assert (knn_i != np.arange(N)[:, None]).all(), "self among the neighbours"
    assert (np.diff(np.sort(knn_i, axis=1), axis=1) > 0).all(), "repeated neighbour"
    if bound is None:
        full = np.empty((N, N))
        np.put_along_axis(full, order, key, 1)
        tol = 2 * U if metric == "jaccard" else 0.0
        for r in range(N):
            kth = key[r, K - 1]
            closer = set(order[r][key[r] < kth - tol].tolist())
            got = set(knn_i[r].tolist())
            assert closer <= got, r
            rest = np.array(sorted(got - closer), dtype=np.int64)
            assert (np.abs(full[r, rest] - kth) <= tol).all(), r
        return 0
    bad = 0
    for r in range(N):
        if set(knn_i[r].tolist()) != set(order[r, :K].tolist()):
            gap = key[r, K] - key[r, K - 1]
            b = max(bound[r, order[r, K - 1]], bound[r, order[r, K]])
            assert gap < 2 * b, (r, gap, b)
            bad += 1
    print(f"{metric}: {bad} rows differ")
    assert bad <= N // 100, bad
    return bad


def _fit_capture(monkeypatch, X, **kw):
    """Fit and return (model, neighbour indices handed to the fuzzy set)."""
    seen = {}
    orig = umap_mod._fuzzy_simplicial_set_t

    def spy(knn_d, knn_i, *a):
        seen["d"], seen["i"] = knn_d.cpu().numpy(), knn_i.cpu().numpy()
        return orig(knn_d, knn_i, *a)

    monkeypatch.setattr(umap_mod, "_fuzzy_simplicial_set_t", spy)
    kw.setdefault("n_epochs", 5)
    model = UMAP(n_neighbors=K, random_state=3, init="random", **kw).fit(DataFrame.from_numpy(X))
    return model, seen


def _graph_case(monkeypatch, metric):
    kw = {"metric_kwds": {"p": 3}} if metric == "minkowski" else {}
    _, seen = _fit_capture(monkeypatch, _metric_data(metric), metric=metric, **kw)
    _check_graph(seen["i"], metric)
    assert np.isfinite(seen["d"]).all() and (np.diff(seen["d"], axis=1) >= 0).all()


# ---------------------------------------------------------------------------
# graph stage
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("metric", GRAPH_METRICS)
def test_graph_stage_matches_scipy(metric, monkeypatch):
    _graph_case(monkeypatch, metric)


@gpu
@pytest.mark.parametrize("metric", GRAPH_METRICS)
def test_graph_stage_matches_scipy_gpu(metric, monkeypatch, kernel_only):
    _graph_case(monkeypatch, metric)


@gpu
def test_graph_is_bit_reproducible_gpu(kernel_only):
    from spark_rapids_ml_amd.ops.knn import knn_topk_metric_sparse

    X = _data()
    a = knn_topk_metric_sparse(X, X, K + 1, "cosine", device="cuda")
    b = knn_topk_metric_sparse(X, X, K + 1, "cosine", device="cuda")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---------------------------------------------------------------------------
# estimator
# ---------------------------------------------------------------------------


@lru_cache(maxsize=None)
def _blocks():
    """3 clusters of 100 rows, each switching on about 60 % of its own 20
    columns: jaccard distance below 1 within a cluster, exactly 1 across."""
    rng = np.random.default_rng(2)
    B = np.zeros((300, 60), dtype=np.float32)
    for c in range(3):
        B[c * 100:(c + 1) * 100, c * 20:(c + 1) * 20] = rng.random((100, 20)) < 0.6
    assert (B.sum(1) > 0).all()
    return B


def _same(A, B):
    return A.shape == B.shape and (sp.csr_matrix(A) != sp.csr_matrix(B)).nnz == 0


def test_jaccard_fit_on_csr():
    """sklearn's trustworthiness (n_neighbors=10, metric='jaccard') of this
    embedding, measured with the CPU path: 0.9342; on the MI355X (HIP SGD,
    not run-to-run deterministic): 0.9264."""
    from sklearn.manifold import trustworthiness

    B = _blocks()
    X = sp.csr_matrix(B)
    model = UMAP(metric="jaccard", n_neighbors=15, random_state=1).fit(DataFrame.from_numpy(X))
    assert isinstance(model.rawData, sp.csr_matrix)
    assert _same(model.rawData, X)
    assert model.embedding.shape == (300, 2) and np.isfinite(model.embedding).all()
    tw = trustworthiness(B != 0, model.embedding, n_neighbors=10, metric="jaccard")
    print(f"trustworthiness[jaccard] = {tw:.6f}")
    assert tw >= 0.9, tw


def test_sparse_and_dense_fits_share_the_graph(monkeypatch):
    rng = np.random.default_rng(4)
    Xd = ((rng.random((200, 80)) < 0.15) * rng.integers(1, 5, (200, 80))).astype(np.float32)
    Xd += rng.random((200, 80)).astype(np.float32) < 0.02  # few ties among integer sums
    Xd[:, 0] += np.arange(200) % 7
    _, s = _fit_capture(monkeypatch, sp.csr_matrix(Xd), metric="manhattan")
    _, d = _fit_capture(monkeypatch, Xd, metric="manhattan")
    # integer data: both paths are exact, so the distances agree to the bit,
    # and the sets wherever the k-th distance is not tied with the (k+1)-th.
    # On a tied row either path may keep any of the tied points: there both
    # sets hold every strictly closer point and the rest lie exactly at the
    # k-th distance (the tie-invariant check used for hamming).
    assert np.array_equal(s["d"], d["d"])
    full = cdist(Xd, Xd, "cityblock")
    np.fill_diagonal(full, np.inf)
    srt = np.sort(full, axis=1)
    untied = srt[:, K - 1] < srt[:, K]
    assert untied.sum() > 50 and (~untied).sum() > 0
    for r in range(200):
        got_s, got_d = set(s["i"][r].tolist()), set(d["i"][r].tolist())
        if untied[r]:
            assert got_s == got_d, r
            continue
        kth = srt[r, K - 1]
        closer = set(np.nonzero(full[r] < kth)[0].tolist())
        for got in (got_s, got_d):
            assert len(got) == K and closer <= got, r
            assert (full[r, sorted(got - closer)] == kth).all(), r


def test_parameter_rules():
    X = _data()[:60]
    dense = np.asarray(X.todense())
    df_s, df_d = DataFrame.from_numpy(X), DataFrame.from_numpy(dense)
    with pytest.raises(ValueError, match="requires sparse CSR"):
        UMAP(enable_sparse_data_optim=True, n_epochs=2).fit(df_d)
    model = UMAP(enable_sparse_data_optim=False, n_epochs=2, init="random").fit(df_s)
    assert isinstance(model.rawData, np.ndarray) and np.array_equal(model.rawData, dense)
    with pytest.raises(ValueError, match="Metric 'jaccard' not supported for dense inputs."):
        UMAP(metric="jaccard", n_epochs=2).fit(df_d)
    with pytest.raises(ValueError, match="Metric 'jaccard' not supported for dense inputs."):
        UMAP(metric="jaccard", n_epochs=2, enable_sparse_data_optim=False).fit(df_s)
    for metric in ("chebyshev", "linf", "correlation"):
        with pytest.raises(ValueError, match="sparse input"):
            UMAP(metric=metric, n_epochs=2).fit(df_s)
    with pytest.raises(ValueError, match="sparse input"):
        UMAP(build_algo="nn_descent", n_epochs=2).fit(df_s)
    Z = X.tolil()
    Z[5, :] = 0
    with pytest.raises(ValueError, match="zero-norm"):
        UMAP(metric="cosine", n_epochs=2).fit(DataFrame.from_numpy(Z.tocsr()))
    Z[5, 3] = -1.0
    with pytest.raises(ValueError, match="non-negative"):
        UMAP(metric="hellinger", n_epochs=2).fit(DataFrame.from_numpy(Z.tocsr()))


def test_resolve_metric_sparse_keyword():
    from spark_rapids_ml_amd.ops.knn import resolve_metric

    assert resolve_metric("jaccard", sparse=True) == ("jaccard", 2.0)
    assert resolve_metric("l1", sparse=True) == ("manhattan", 2.0)
    assert resolve_metric("minkowski", 3, sparse=True) == ("minkowski", 3.0)
    with pytest.raises(ValueError, match="'chebyshev'.*sparse input"):
        resolve_metric("linf", sparse=True)
    with pytest.raises(ValueError, match="not supported for dense inputs"):
        resolve_metric("jaccard")
    assert resolve_metric("chebyshev") == ("chebyshev", 2.0)


def test_save_load_transform(monkeypatch, tmp_model_path):
    X = _data()
    model = UMAP(n_neighbors=K, n_epochs=5, random_state=3, metric="manhattan").fit(
        DataFrame.from_numpy(X)
    )
    Q = X[:40] * 1.5
    seen = []
    orig = umap_mod.knn_topk_metric_sparse

    def spy(*a, **k):
        out = orig(*a, **k)
        seen.append((out[0].cpu().numpy(), out[1].cpu().numpy()))
        return out

    monkeypatch.setattr(umap_mod, "knn_topk_metric_sparse", spy)
    before = np.asarray(model.transform(DataFrame.from_numpy(Q))["embedding"])
    model.save(tmp_model_path)
    loaded = UMAPModel.load(tmp_model_path)
    assert isinstance(loaded.rawData, sp.csr_matrix) and _same(loaded.rawData, X)
    assert loaded.rawData.dtype == np.float32
    after = np.asarray(loaded.transform(DataFrame.from_numpy(Q))["embedding"])
    # a dense batch against the sparse model is converted to CSR
    dense = np.asarray(loaded.transform(DataFrame.from_numpy(np.asarray(Q.todense())))["embedding"])
    for out in (before, after, dense):
        assert out.shape == (40, 2) and np.isfinite(out).all()
    # the kNN stage of transform is deterministic on every device: the same
    # neighbours and distances before saving, after loading and for the dense
    # batch, and they are the manhattan neighbours
    assert len(seen) == 3
    for dist, idx in seen[1:]:
        assert np.array_equal(dist, seen[0][0]) and np.array_equal(idx, seen[0][1])
    ref = cdist(Q.toarray().astype(np.float64), X.toarray().astype(np.float64), "cityblock")
    m = int(np.diff(X.indptr).max())
    want = np.sort(ref, axis=1)[:, :K]
    bound = 2 * _gamma(2 * m + 6) * (np.abs(Q.toarray()).sum(1)[:, None] + np.abs(X.toarray()).sum(1).max())
    assert (np.abs(seen[0][0] - want) <= bound).all()
    # the SGD that follows is the torch generator's on the CPU, bit-identical
    # run to run; the HIP kernel's is Hogwild and is not
    if not torch.cuda.is_available():
        assert np.array_equal(before, after) and np.array_equal(dense, after)


def _dist_sparse_fit(_):
    from spark_rapids_ml_amd.parallel.context import get_comm

    comm = get_comm()
    X = _data()[:120]
    lo, hi = (0, 70) if comm.rank == 0 else (70, 120)  # uneven shards
    model = UMAP(n_neighbors=10, n_epochs=3, random_state=3, init="random", metric="jaccard").fit(
        DataFrame.from_numpy(X[lo:hi])
    )
    raw = model.rawData
    return sp.issparse(raw), raw.toarray(), model.embedding


def test_two_rank_fit_gathers_csr():
    results = run_distributed(_dist_sparse_fit, world_size=2, args=(None,))
    want = _data()[:120].toarray()
    for is_sparse, raw, emb in results:
        assert is_sparse and np.array_equal(raw, want)
        assert emb.shape == (120, 2) and np.isfinite(emb).all()
    assert np.array_equal(results[0][2], results[1][2])
