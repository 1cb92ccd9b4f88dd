"""UMAP(metric=...): parameter handling, the kNN graph stage against scipy,
embedding quality and save -> load -> transform under a non-euclidean metric.

The estimator runs on the process's device, so every unmarked test runs on
the CPU path where there is no GPU; the `gpu`-marked twins additionally
forbid the torch kNN path (`kernel_only`).
"""

from functools import lru_cache

import numpy as np
import pytest
import torch
from scipy.spatial.distance import cdist

from spark_rapids_ml_amd import UMAP, UMAPModel
from spark_rapids_ml_amd.data import DataFrame
from spark_rapids_ml_amd.models import umap as umap_mod
from spark_rapids_ml_amd.ops import torch_ref

gpu = pytest.mark.gpu
U = 2.0 ** -24
N, D, K = 500, 24, 15
SCIPY_NAME = {"manhattan": "cityblock"}
GRAPH_METRICS = ["manhattan", "chebyshev", "canberra", "hamming", "cosine", "correlation"]


@pytest.fixture
def kernel_only(monkeypatch):
    def _no(*a, **k):
        raise AssertionError("torch fallback taken on the GPU")

    monkeypatch.setattr(torch_ref, "knn_topk_metric", _no)
    assert torch.cuda.is_available()


def _gamma(n):
    return n * U / (1.0 - n * U)


@lru_cache(maxsize=None)
def _graph_data(metric):
    rng = np.random.default_rng(11)
    if metric == "hamming":
        return (rng.random((N, D)) < 0.5).astype(np.float32)
    return rng.normal(size=(N, D)).astype(np.float32)


@lru_cache(maxsize=None)
def _graph_reference(metric, p=2.0):
    """(sorted neighbour indices [N, N-1] without self, their f64 distances,
    per-entry error bound of an f32 evaluation as (rel, abs)).

    manhattan: fl(q-x) U + gamma_D for the sum. chebyshev: U. canberra: 5U per
    term + gamma_D (tests/test_pairwise_metrics.py). minkowski p=3: the bound
    derived there, computed from this data. cosine: (2D+7)U absolute;
    correlation adds 2 gamma_D kappa with kappa = max mean|x| sqrt(D)/||x-mean||
    (same derivations). hamming is exact."""
    X = _graph_data(metric)
    X64 = X.astype(np.float64)
    kw = {"p": p} if metric == "minkowski" else {}
    Dm = cdist(X64, X64, SCIPY_NAME.get(metric, metric), **kw)
    np.fill_diagonal(Dm, np.inf)  # self excluded
    order = np.argsort(Dm, axis=1, kind="stable")[:, : N - 1]
    dist = np.take_along_axis(Dm, order, 1)
    rel, abs_ = 0.0, 0.0
    if metric == "manhattan":
        rel = _gamma(D + 1)
    elif metric == "chebyshev":
        rel = U
    elif metric == "canberra":
        rel = _gamma(D + 6)
    elif metric == "minkowski":
        from tests.test_pairwise_metrics import _lp_bound

        rel = _lp_bound(X, X, p)
    elif metric in ("cosine", "correlation"):
        abs_ = (2 * D + 7) * U
        if metric == "correlation":
            c = X64 - X64.mean(1, keepdims=True)
            abs_ += 2 * _gamma(D) * (np.abs(X64).mean(1) * np.sqrt(D) / np.linalg.norm(c, axis=1)).max()
    return order, dist, (rel, abs_)


def _check_graph(knn_i, metric, p=2.0):
    """Neighbour sets equal scipy's per row. A row may differ only where the
    reference's k-th and (k+1)-th distances are closer than twice the error
    bound (either may move by the bound); at most 1 % of rows may.

    hamming on 0/1 data has integer counts out of D = 24, so nearly every row
    ties at the k-th distance and no set is THE neighbour set; f32 counts are
    exact, so the check there is the tie-invariant exact one: every point
    strictly closer than the reference's k-th distance is present and every
    other returned point lies exactly at that distance."""
    order, dist, (rel, abs_) = _graph_reference(metric, p)
    knn_i = np.asarray(knn_i)
    n = knn_i.shape[0]
    assert knn_i.shape == (n, K)
    assert (knn_i != np.arange(n)[:, None]).all(), "self among the neighbours"
    assert (np.diff(np.sort(knn_i, axis=1), axis=1) > 0).all(), "repeated neighbour"
    if metric == "hamming":
        X = _graph_data(metric)
        for r in range(n):
            kth = dist[r, K - 1]
            closer = set(order[r][dist[r] < kth].tolist())
            got = set(knn_i[r].tolist())
            assert closer <= got
            rest = np.array(sorted(got - closer), dtype=np.int64)
            assert ((X[rest] != X[r]).mean(axis=1) == kth).all()
        return 0
    bad = 0
    for r in range(n):
        if set(knn_i[r].tolist()) != set(order[r, :K].tolist()):
            gap = dist[r, K] - dist[r, K - 1]
            assert gap < 2 * (rel * dist[r, K] + abs_), (r, gap)
            bad += 1
    assert bad <= n // 100, bad
    return bad


def _fit_capture(monkeypatch, X, **kw):
    """Fit and return (model, neighbour indices handed to the fuzzy set)."""
    seen = {}
    orig = umap_mod._fuzzy_simplicial_set_t

    def spy(knn_d, knn_i, *a):
        seen["d"], seen["i"] = knn_d.cpu().numpy(), knn_i.cpu().numpy()
        return orig(knn_d, knn_i, *a)

    monkeypatch.setattr(umap_mod, "_fuzzy_simplicial_set_t", spy)
    model = UMAP(n_neighbors=K, n_epochs=5, random_state=3, init="random", **kw).fit(
        DataFrame.from_numpy(X)
    )
    return model, seen


# ---------------------------------------------------------------------------
# parameters and errors
# ---------------------------------------------------------------------------


def test_every_documented_name_resolves():
    canon = {"l1": "manhattan", "cityblock": "manhattan", "taxicab": "manhattan",
             "l2": "euclidean", "linf": "chebyshev", "minkowski": "euclidean"}
    for name in ("l1 cityblock taxicab manhattan euclidean l2 sqeuclidean canberra minkowski "
                 "chebyshev linf cosine correlation hellinger hamming").split():
        est = UMAP(metric=name)
        assert est.cuml_params["metric"] == name
        assert est._metric()[0] == canon.get(name, name)
    assert UMAP(metric="minkowski", metric_kwds={"p": 3})._metric() == ("minkowski", 3.0)
    assert UMAP(metric="minkowski", metric_kwds={"p": 1})._metric()[0] == "manhattan"


def test_metric_errors():
    X = _graph_data("cosine")[:60]
    df = DataFrame.from_numpy(X)
    with pytest.raises(ValueError, match="Metric 'jaccard' not supported for dense inputs."):
        UMAP(metric="jaccard", n_epochs=2).fit(df)
    with pytest.raises(ValueError, match="accepted: canberra"):
        UMAP(metric="mahalanobis")
    with pytest.raises(ValueError, match="finite and > 0"):
        UMAP(metric="minkowski", metric_kwds={"p": 0}, n_epochs=2).fit(df)
    Z = X.copy()
    Z[5] = 0.0
    with pytest.raises(ValueError, match="zero-norm"):
        UMAP(metric="cosine", n_epochs=2).fit(DataFrame.from_numpy(Z))
    Z[5] = 1.5
    with pytest.raises(ValueError, match="constant"):
        UMAP(metric="correlation", n_epochs=2).fit(DataFrame.from_numpy(Z))
    with pytest.raises(ValueError, match="non-negative"):
        UMAP(metric="hellinger", n_epochs=2).fit(df)


@pytest.mark.parametrize("metric", ["manhattan", "chebyshev", "canberra", "hamming", "hellinger"])
def test_nn_descent_needs_an_l2_metric(metric):
    X = np.abs(_graph_data("cosine")[:60])
    with pytest.raises(ValueError, match="nn_descent"):
        UMAP(metric=metric, build_algo="nn_descent", n_epochs=2).fit(DataFrame.from_numpy(X))


def test_nn_descent_cosine_builds_on_unit_rows():
    X = _graph_data("cosine")
    model = UMAP(metric="cosine", build_algo="nn_descent", n_neighbors=K, n_epochs=5,
                 random_state=3).fit(DataFrame.from_numpy(X))
    assert np.isfinite(model.embedding).all()


def test_drop_self_handles_displaced_self_match():
    i = torch.tensor([[0, 5, 6], [7, 1, 8], [4, 5, 6]])
    d = torch.tensor([[0.0, 1.0, 2.0], [0.0, 0.0, 3.0], [1.0, 2.0, 3.0]])
    dd, ii = umap_mod._drop_self(d, i)
    assert ii.tolist() == [[5, 6], [7, 8], [4, 5]]
    assert dd.tolist() == [[1.0, 2.0], [0.0, 3.0], [1.0, 2.0]]


# ---------------------------------------------------------------------------
# graph stage
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("metric", GRAPH_METRICS)
def test_cpu_torch_reference_stays_within_the_cap(metric):
    """The data chosen keeps the f32 torch reference alone within the 1 % cap."""
    X = torch.from_numpy(_graph_data(metric))
    _, idx = torch_ref.knn_topk_metric(X, X, K + 1, metric)
    keep = idx != torch.arange(N)[:, None]
    has_self = (~keep).any(dim=1)
    keep[~has_self, -1] = False
    _check_graph(idx[keep].reshape(N, K).numpy(), metric)


@pytest.mark.parametrize("metric", GRAPH_METRICS)
def test_graph_stage_matches_scipy(metric, monkeypatch):
    _, seen = _fit_capture(monkeypatch, _graph_data(metric), metric=metric)
    _check_graph(seen["i"], metric)


def test_graph_stage_honours_metric_kwds_p(monkeypatch):
    X = _graph_data("minkowski")
    _, seen = _fit_capture(monkeypatch, X, metric="minkowski", metric_kwds={"p": 3})
    _check_graph(seen["i"], "minkowski", 3.0)
    # and p = 3 is not what p = 2 would have given
    order2 = _graph_reference("minkowski", 2.0)[0][:, :K]
    assert any(set(a) != set(b) for a, b in zip(seen["i"].tolist(), order2.tolist()))


@gpu
@pytest.mark.parametrize("metric", GRAPH_METRICS)
def test_graph_stage_matches_scipy_gpu(metric, monkeypatch, kernel_only):
    _, seen = _fit_capture(monkeypatch, _graph_data(metric), metric=metric)
    _check_graph(seen["i"], metric)


@gpu
def test_graph_stage_honours_metric_kwds_p_gpu(monkeypatch, kernel_only):
    _, seen = _fit_capture(monkeypatch, _graph_data("minkowski"), metric="minkowski",
                           metric_kwds={"p": 3})
    _check_graph(seen["i"], "minkowski", 3.0)


# ---------------------------------------------------------------------------
# quality
# ---------------------------------------------------------------------------

# euclidean fit of the blobs case on the parent commit, seeds 7..11
BASELINE_CPU = [0.941634, 0.941707, 0.940570, 0.940596, 0.940126]
BASELINE_GPU = [0.939809, 0.940685, 0.939939, 0.940703, 0.940275]


def _bar():
    base = BASELINE_GPU if torch.cuda.is_available() else BASELINE_CPU
    return min(base) - (max(base) - min(base))


def _quality(metric):
    """Trustworthiness (n_neighbors=10, under the fitted metric) of the
    project's blobs case fitted with `metric`.

    Baseline: trustworthiness of the euclidean fit on the parent commit over
    seeds 7..11 (n_epochs=150, n_neighbors=15), measured per device because
    the SGD differs (torch generator on the CPU, hash RNG in the HIP kernel):
      CPU 0.941634 0.941707 0.940570 0.940596 0.940126 -> min 0.940126,
          spread 0.001581, bar 0.938545
      GPU 0.939809 0.940685 0.939939 0.940703 0.940275 -> min 0.939809,
          spread 0.000894, bar 0.938915
    The bar is min - spread. For orientation, the floor the project already
    asserts for this data is 0.92.

    Measured with this test's seed (7): CPU manhattan 0.939793, cosine
    0.940808 (both above the CPU bar). MI355X cosine 0.940405 (above),
    manhattan 0.937762, and 0.938541 in a second run of the whole suite (the
    HIP SGD is Hogwild, not run-to-run deterministic): BELOW the GPU bar by
    0.0004 to 0.0012, so the manhattan case fails on the GPU. Over seeds
    7..11 manhattan gives 0.937762 0.939211 0.939804 0.939563 0.938780 there. The manhattan kNN graph itself equals
    scipy's (test_graph_stage_matches_scipy); the embedding scores about
    0.002 lower under manhattan than the euclidean fit does under euclidean
    on both devices (CPU 0.939793 against 0.941634), which is wider than the
    euclidean seed spread the bar allows on the GPU."""
    from sklearn.datasets import make_blobs
    from sklearn.manifold import trustworthiness

    X, _ = make_blobs(n_samples=2000, n_features=24, centers=6, cluster_std=0.6, random_state=0)
    X = X.astype(np.float32)
    model = UMAP(n_neighbors=15, n_epochs=150, random_state=7, metric=metric).fit(
        DataFrame.from_numpy(X)
    )
    tw = trustworthiness(X, model.embedding, n_neighbors=10, metric=metric)
    print(f"trustworthiness[{metric}] = {tw:.6f}, bar = {_bar():.6f}")
    assert tw >= _bar(), (tw, _bar())


@pytest.mark.parametrize("metric", ["manhattan", "cosine"])
def test_blobs_quality(metric):
    _quality(metric)


# ---------------------------------------------------------------------------
# save -> load -> transform
# ---------------------------------------------------------------------------


def _persistence(monkeypatch, path):
    X = _graph_data("cosine")
    model = UMAP(n_neighbors=K, n_epochs=5, random_state=3, metric="cosine").fit(
        DataFrame.from_numpy(X)
    )
    model.save(path)
    loaded = UMAPModel.load(path)
    assert loaded.getOrDefault("metric") == "cosine"

    # new rows, each rescaled by its own factor: cosine ignores the scale,
    # euclidean does not
    rng = np.random.default_rng(21)
    Q = (rng.normal(size=(64, D)) * rng.uniform(0.05, 20.0, size=(64, 1))).astype(np.float32)
    seen = {}
    orig = umap_mod.knn_topk_metric

    def spy(*a, **k):
        seen["d"], seen["i"] = orig(*a, **k)
        return seen["d"], seen["i"]

    monkeypatch.setattr(umap_mod, "knn_topk_metric", spy)
    out = np.asarray(loaded.transform(DataFrame.from_numpy(Q))["embedding"])
    assert out.shape == (64, 2) and np.isfinite(out).all()

    Dm = cdist(Q.astype(np.float64), X.astype(np.float64), "cosine")
    order = np.argsort(Dm, axis=1, kind="stable")
    dist = np.take_along_axis(Dm, order, 1)
    got = seen["i"].cpu().numpy()
    bound = (2 * D + 7) * U
    for r in range(64):
        if set(got[r].tolist()) != set(order[r, :K].tolist()):
            assert dist[r, K] - dist[r, K - 1] < 2 * bound
    eu = np.argsort(cdist(Q.astype(np.float64), X.astype(np.float64)), axis=1)[:, :K]
    assert sum(set(a) != set(b) for a, b in zip(eu.tolist(), order[:, :K].tolist())) > 32


def test_save_load_transform_uses_the_fitted_metric(monkeypatch, tmp_model_path):
    _persistence(monkeypatch, tmp_model_path)


@gpu
def test_save_load_transform_uses_the_fitted_metric_gpu(monkeypatch, tmp_model_path, kernel_only):
    _persistence(monkeypatch, tmp_model_path)
