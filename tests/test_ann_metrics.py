"""ANN metrics: sqeuclidean, cosine and inner_product against numpy float64
brute force (the reference supports these for ivfflat and ivfpq,
knn.py:1007-1010). Expected values never come from the code under test."""

import numpy as np
import pytest

from spark_rapids_ml_amd import ApproximateNearestNeighbors, NearestNeighbors
from spark_rapids_ml_amd.data import DataFrame

NEW_METRICS = ["sqeuclidean", "cosine", "inner_product"]


def _data(n, d=16, seed=0):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(n, d)).astype(np.float32)


def brute_force(Q, X, metric, k):
    """Reported distance under `metric` in float64, best first:
    (dist [nq, k], idx [nq, k])."""
    Q = Q.astype(np.float64)
    X = X.astype(np.float64)
    if metric == "inner_product":
        D = Q @ X.T
        idx = np.argsort(-D, axis=1, kind="stable")[:, :k]
    else:
        if metric == "cosine":
            Qn = Q / np.linalg.norm(Q, axis=1, keepdims=True)
            Xn = X / np.linalg.norm(X, axis=1, keepdims=True)
            D = 1.0 - Qn @ Xn.T
        else:
            D = ((Q[:, None, :] - X[None, :, :]) ** 2).sum(axis=2)
            if metric in ("euclidean", "l2"):
                D = np.sqrt(D)
        idx = np.argsort(D, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(D, idx, axis=1), idx


def _kneighbors(X, Q, k, algo, params, metric, **kw):
    model = ApproximateNearestNeighbors(
        k=k, algorithm=algo, algoParams=params, metric=metric, **kw
    ).fit(DataFrame.from_numpy(X))
    _, _, knn_df = model.kneighbors(DataFrame.from_numpy(Q))
    return np.asarray(knn_df["indices"]), np.asarray(knn_df["distances"])


def _recall(idx, ref_idx):
    hits = sum(len(set(a.tolist()) & set(b.tolist())) for a, b in zip(idx, ref_idx))
    return hits / ref_idx.size


def assert_exact(idx, dist, Q, X, metric, k):
    ref_d, ref_i = brute_force(Q, X, metric, k)
    assert idx.shape == ref_i.shape
    for row, ref_row in zip(idx, ref_i):
        assert set(row.tolist()) == set(ref_row.tolist())
    np.testing.assert_allclose(dist, ref_d, rtol=1e-4, atol=1e-4)
    if metric == "inner_product":
        assert (np.diff(dist, axis=1) <= 0).all()
    else:
        assert (np.diff(dist, axis=1) >= 0).all()


# 1 -------------------------------------------------------------------------
@pytest.mark.parametrize("metric", NEW_METRICS)
def test_ivfflat_full_probe_is_exact(metric):
    X = _data(500)
    Q = X[:50]
    idx, dist = _kneighbors(X, Q, 5, "ivfflat", {"nlist": 8, "nprobe": 8}, metric)
    assert_exact(idx, dist, Q, X, metric, 5)


# 2 -------------------------------------------------------------------------
def test_cosine_ignores_row_scale():
    X = _data(500)
    Q = X[:50]
    scale = np.random.default_rng(1).uniform(0.5, 20.0, size=(500, 1)).astype(np.float32)
    params = {"nlist": 8, "nprobe": 8}
    idx, _ = _kneighbors(X, Q, 5, "ivfflat", params, "cosine")
    idx_s, _ = _kneighbors(X * scale, (X * scale)[:50], 5, "ivfflat", params, "cosine")
    np.testing.assert_array_equal(idx, idx_s)


# 3 -------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "inner_product"])
@pytest.mark.parametrize("algo,params", [
    ("ivfflat", {"nlist": 32, "nprobe": 8}),
    ("ivfpq", {"nlist": 32, "nprobe": 32, "refine_ratio": 4.0}),
])
def test_recall_at_partial_probe(algo, params, metric):
    X = _data(2000)
    Q = X[:100]
    idx, _ = _kneighbors(X, Q, 10, algo, params, metric)
    _, ref_i = brute_force(Q, X, metric, 10)
    rec = _recall(idx, ref_i)
    assert rec > 0.7, f"{algo} {metric} recall {rec}"


# 4 -------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "inner_product"])
def test_ivfpq_exact_limit(metric):
    X = _data(400)
    Q = X[:40]
    # k_cand = k * refine_ratio = n: the refine re-ranks every item
    params = {"nlist": 8, "nprobe": 8, "refine_ratio": 80.0}
    idx, dist = _kneighbors(X, Q, 5, "ivfpq", params, metric)
    assert_exact(idx, dist, Q, X, metric, 5)


# 5 -------------------------------------------------------------------------
def test_cagra_rejects_cosine():
    X = _data(200)
    model = ApproximateNearestNeighbors(k=3, algorithm="cagra", metric="cosine").fit(
        DataFrame.from_numpy(X)
    )
    with pytest.raises(ValueError):
        model.kneighbors(DataFrame.from_numpy(X[:5]))


def test_set_metric_rejects_unknown():
    with pytest.raises(ValueError):
        ApproximateNearestNeighbors().setMetric("bogus")


def test_constructor_metric_rejected_at_kneighbors():
    X = _data(100)
    model = ApproximateNearestNeighbors(k=3, metric="bogus").fit(DataFrame.from_numpy(X))
    with pytest.raises(ValueError):
        model.kneighbors(DataFrame.from_numpy(X[:5]))


@pytest.mark.parametrize(
    "metric", ["euclidean", "l2", "sqeuclidean", "inner_product", "cosine"]
)
def test_get_metric_round_trips(metric):
    est = ApproximateNearestNeighbors().setMetric(metric)
    assert est.getMetric() == metric
    assert ApproximateNearestNeighbors(metric=metric).getMetric() == metric
    assert ApproximateNearestNeighbors().getMetric() == "euclidean"


# 6 -------------------------------------------------------------------------
def _dist_ann_ip():
    from spark_rapids_ml_amd.parallel.context import get_comm

    comm = get_comm()
    rng = np.random.default_rng(0)
    X = rng.normal(size=(600, 16)).astype(np.float32)
    Q = rng.normal(size=(30, 16)).astype(np.float32)
    ids = np.arange(600, dtype=np.int64)
    df = DataFrame({
        "features": X[comm.rank :: comm.world_size],
        "id": ids[comm.rank :: comm.world_size],
    })
    qdf = DataFrame({"features": Q[comm.rank :: comm.world_size]})
    model = ApproximateNearestNeighbors(
        k=8, algorithm="ivfflat", algoParams={"nlist": 8, "nprobe": 8},
        idCol="id", metric="inner_product",
    ).fit(df)
    _, _, knn_df = model.kneighbors(qdf)
    return np.asarray(knn_df["indices"]), np.asarray(knn_df["distances"])


def test_inner_product_distributed_merge():
    """Two ranks, full probe: the merged neighbours are the brute-force
    inner-product neighbours over the union of the shards, largest dot
    first (pins the descending merge)."""
    from tests.dist_utils import run_distributed

    results = run_distributed(_dist_ann_ip, world_size=2)
    rng = np.random.default_rng(0)
    X = rng.normal(size=(600, 16)).astype(np.float32)
    Q = rng.normal(size=(30, 16)).astype(np.float32)
    for r, (idx, dist) in enumerate(results):
        assert_exact(idx, dist, Q[r::2], X, "inner_product", 8)


def test_inner_product_pads_with_minus_inf():
    """Fewer items than k: the empty slots report -inf and id -1, after the
    real neighbours."""
    X = _data(3)
    Q = _data(4, seed=1)
    idx, dist = _kneighbors(X, Q, 5, "ivfflat", {"nlist": 1, "nprobe": 1}, "inner_product")
    ref_d, ref_i = brute_force(Q, X, "inner_product", 3)
    np.testing.assert_array_equal(idx[:, :3], ref_i)
    np.testing.assert_allclose(dist[:, :3], ref_d, rtol=1e-4, atol=1e-4)
    assert (idx[:, 3:] == -1).all()
    assert np.isneginf(dist[:, 3:]).all()


def test_sqeuclidean_pads_with_plus_inf():
    X = _data(3)
    Q = _data(4, seed=1)
    idx, dist = _kneighbors(X, Q, 5, "ivfflat", {"nlist": 1, "nprobe": 1}, "sqeuclidean")
    assert (idx[:, 3:] == -1).all()
    assert np.isposinf(dist[:, 3:]).all()


def test_cosine_zero_vector_is_half_from_everything():
    X = _data(50)
    Q = np.zeros((1, 16), dtype=np.float32)
    _, dist = _kneighbors(X, Q, 5, "ivfflat", {"nlist": 2, "nprobe": 2}, "cosine")
    np.testing.assert_allclose(dist, 0.5, rtol=1e-5)


def test_cagra_sqeuclidean_reports_squared():
    X = _data(600)
    Q = X[:20]
    params = {"graph_degree": 32, "itopk_size": 128, "max_iterations": 10}
    idx, d_sq = _kneighbors(X, Q, 5, "cagra", params, "sqeuclidean")
    idx_e, d_e = _kneighbors(X, Q, 5, "cagra", params, "euclidean")
    np.testing.assert_array_equal(idx, idx_e)
    true_sq = ((Q[:, None, :].astype(np.float64) - X[idx].astype(np.float64)) ** 2).sum(2)
    np.testing.assert_allclose(d_sq, true_sq, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(d_e, np.sqrt(true_sq), rtol=1e-4, atol=1e-4)


# 7 -------------------------------------------------------------------------
def test_exact_knn_unchanged():
    """The exact path shares the partial merge; it keeps the Euclidean
    convention (passes before and after the metric work)."""
    from sklearn.neighbors import NearestNeighbors as SkNN

    X = _data(700, d=12, seed=3)
    Q = _data(40, d=12, seed=4)
    model = NearestNeighbors(k=6).fit(DataFrame.from_numpy(X))
    _, _, knn_df = model.kneighbors(DataFrame.from_numpy(Q))
    sk_d, sk_i = SkNN(n_neighbors=6, algorithm="brute").fit(X).kneighbors(Q)
    np.testing.assert_array_equal(np.asarray(knn_df["indices"]), sk_i)
    np.testing.assert_allclose(np.asarray(knn_df["distances"]), sk_d, rtol=1e-4, atol=1e-4)
