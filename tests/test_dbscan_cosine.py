"""DBSCAN metric="cosine" against sklearn's brute-force cosine DBSCAN
(the reference documents {'euclidean', 'cosine'}, clustering.py:761)."""

import numpy as np
import pytest
from sklearn.cluster import DBSCAN as SkDBSCAN
from sklearn.metrics import adjusted_rand_score

from spark_rapids_ml_amd import DBSCAN
from spark_rapids_ml_amd.data import DataFrame

EPS, MIN_SAMPLES = 0.05, 5


def cosine_fixture(seed=0, n=300, d=8):
    """Three tight direction bundles with wildly varying row lengths (so
    Euclidean distance at this eps finds nothing) plus 10 noise rows."""
    rng = np.random.default_rng(seed)
    dirs = rng.normal(size=(3, d))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    X = dirs[rng.integers(0, 3, size=n)] + 0.02 * rng.normal(size=(n, d))
    X *= rng.uniform(0.5, 20.0, size=(n, 1))
    X[:10] = rng.normal(size=(10, d))
    return X.astype(np.float32)


def assert_no_edge_near_eps(X):
    """No pair's float64 cosine distance lies in [eps/2, 2*eps]: rounding
    cannot flip an edge, so the labelling is unique up to renaming."""
    Xn = X.astype(np.float64)
    Xn /= np.linalg.norm(Xn, axis=1, keepdims=True)
    D = 1.0 - Xn @ Xn.T
    assert not ((D >= EPS / 2) & (D <= 2 * EPS)).any()


def check_against_sklearn(X, algorithm):
    assert_no_edge_near_eps(X)
    sk = SkDBSCAN(eps=EPS, min_samples=MIN_SAMPLES, metric="cosine", algorithm="brute")
    expected = sk.fit_predict(X.astype(np.float64))
    assert len(set(expected[expected >= 0])) == 3
    assert int((expected == -1).sum()) == 10
    model = DBSCAN(
        eps=EPS, min_samples=MIN_SAMPLES, metric="cosine", algorithm=algorithm
    ).fit(DataFrame.from_numpy(X))
    labels = np.asarray(model.transform(DataFrame.from_numpy(X))["prediction"])
    np.testing.assert_array_equal(labels == -1, expected == -1)
    assert adjusted_rand_score(expected, labels) == 1.0


@pytest.mark.parametrize("algorithm", ["brute", "rbc"])
def test_cosine_matches_sklearn(algorithm):
    check_against_sklearn(cosine_fixture(), algorithm)


def test_cosine_zero_row_raises():
    X = cosine_fixture()
    X[17] = 0.0
    model = DBSCAN(eps=EPS, min_samples=MIN_SAMPLES, metric="cosine").fit(
        DataFrame.from_numpy(X)
    )
    with pytest.raises(ValueError):
        model.transform(DataFrame.from_numpy(X))


def test_unknown_metric_raises():
    X = cosine_fixture()
    model = DBSCAN(eps=EPS, min_samples=MIN_SAMPLES, metric="manhattan").fit(
        DataFrame.from_numpy(X)
    )
    with pytest.raises(ValueError):
        model.transform(DataFrame.from_numpy(X))
