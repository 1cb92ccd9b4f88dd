"""CAGRA model layer on the CPU: the kept index, the search algoParams, and a
plain-Python model of the search that the `cagra_search` kernel implements
(tests/test_cagra_search_gpu.py imports it and compares the kernel to it)."""

import numpy as np
import pytest
import torch

from spark_rapids_ml_amd import ApproximateNearestNeighbors
from spark_rapids_ml_amd.data import DataFrame
from spark_rapids_ml_amd.models import knn


def cagra_search_model(q, X, G, seeds, k, itopk, width, max_it):
    """The specified search for one query. Order is (key, id); a key is the
    f32 value of the float64 squared distance (exact for integer data).
    Returns (keys [k] f32, ids [k] i64, (iterations, evaluations))."""
    n = X.shape[0]
    key = ((X.astype(np.float64) - q.astype(np.float64)) ** 2).sum(1).astype(np.float32)
    visited, expanded = set(), set()

    def fresh(ids):
        out = []
        for j in ids:
            j = int(j)
            if 0 <= j < n and j not in visited:
                visited.add(j)
                out.append((float(key[j]), j))
        return out

    cands = fresh(seeds)
    evals = len(cands)
    lst = sorted(cands)[:itopk]
    iters = 0
    for _ in range(max_it):
        parents = [j for _, j in lst if j not in expanded][:width]
        if not parents:
            break
        iters += 1
        expanded.update(parents)
        cands = fresh(G[parents].reshape(-1))
        evals += len(cands)
        lst = sorted(lst + cands)[:itopk]
    keys = np.full(k, np.inf, dtype=np.float32)
    ids = np.full(k, -1, dtype=np.int64)
    for i, (kv, j) in enumerate(lst[:k]):
        keys[i], ids[i] = kv, j
    return keys, ids, (iters, evals)


def brute_force(Q, X, k):
    d2 = ((Q[:, None, :].astype(np.float64) - X[None].astype(np.float64)) ** 2).sum(2)
    return np.argsort(d2, axis=1, kind="stable")[:, :k]


def recall(found, truth):
    return float(np.mean([len(set(f) & set(t)) / len(t) for f, t in zip(found, truth)]))


def _data(n, d, seed=0):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(n, d)).astype(np.float32)


def _fit(X, k, params, **kw):
    return ApproximateNearestNeighbors(
        k=k, algorithm="cagra", algoParams=params, **kw
    ).fit(DataFrame.from_numpy(X))


def _indices(model, Q):
    _, _, res = model.kneighbors(DataFrame.from_numpy(Q))
    return np.asarray(res["indices"]), np.asarray(res["distances"])


@pytest.fixture
def descent_calls(monkeypatch):
    calls = []
    real = knn._nn_descent

    def spy(*args, **kwargs):
        calls.append(1)
        return real(*args, **kwargs)

    monkeypatch.setattr(knn, "_nn_descent", spy)
    return calls


def test_index_is_built_once_per_build_parameters(descent_calls, monkeypatch):
    monkeypatch.delenv("SRML_ANN_CACHE", raising=False)
    X = _data(600, 8)
    Q = X[:10]
    model = _fit(X, 5, {"graph_degree": 16, "itopk_size": 64})
    first = _indices(model, Q)
    second = _indices(model, Q)
    assert len(descent_calls) == 1
    np.testing.assert_array_equal(first[0], second[0])
    np.testing.assert_array_equal(first[1], second[1])
    # search parameters are not part of the index
    model._set_params(algoParams={"graph_degree": 16, "itopk_size": 96, "search_width": 2,
                                  "max_iterations": 5})
    _indices(model, Q)
    assert len(descent_calls) == 1
    model._set_params(algoParams={"graph_degree": 24, "itopk_size": 96})
    _indices(model, Q)
    assert len(descent_calls) == 2


def test_ann_cache_off_builds_every_time(descent_calls, monkeypatch):
    monkeypatch.setenv("SRML_ANN_CACHE", "0")
    X = _data(600, 8)
    model = _fit(X, 5, {"graph_degree": 16})
    _indices(model, X[:10])
    _indices(model, X[:10])
    assert len(descent_calls) == 2


def test_itopk_size_is_rounded_up_and_checked_against_k(descent_calls):
    X = _data(600, 8)
    model = _fit(X, 40, {"graph_degree": 16, "itopk_size": 8})
    with pytest.raises(ValueError, match="itopk_size"):
        model.kneighbors(DataFrame.from_numpy(X[:4]))
    assert len(descent_calls) == 0  # raised before any work
    model = _fit(X, 64, {"graph_degree": 16, "itopk_size": 33})  # rounds up to 64
    idx, _ = _indices(model, X[:4])
    assert idx.shape == (4, 64)
    assert knn._cagra_search_params({"itopk_size": 33}, 64) == (64, 8, 18)
    assert knn._cagra_search_params({"itopk_size": 128, "max_iterations": 10}, 10) == (128, 16, 10)
    assert knn._cagra_search_params({"search_width": 1}, 10) == (64, 1, 74)


def test_search_width_reaches_the_search(monkeypatch):
    widths_seen = []
    real = knn._graph_beam_search

    def spy(*args, **kwargs):
        widths_seen.append(kwargs.get("expand"))
        return real(*args, **kwargs)

    monkeypatch.setattr(knn, "_graph_beam_search", spy)
    X = _data(2000, 16)
    Q = X[:100]
    truth = brute_force(Q, X, 10)
    base = {"graph_degree": 16, "itopk_size": 64}
    model = _fit(X, 10, base)
    default_idx, _ = _indices(model, Q)
    assert widths_seen == [8]  # the default, max(4, itopk_size // 8)
    model._set_params(algoParams={**base, "search_width": 1, "max_iterations": 1})
    narrow_idx, _ = _indices(model, Q)
    assert any(set(a) != set(b) for a, b in zip(default_idx, narrow_idx))
    recalls, found = [], {}
    for width in (1, 2, 4, 8, 16):
        model._set_params(algoParams={**base, "search_width": width, "max_iterations": 8})
        found[width] = _indices(model, Q)[0]
        recalls.append(recall(found[width], truth))
    assert widths_seen == [8, 1, 1, 2, 4, 8, 16]
    print("recall@10 by search_width 1, 2, 4, 8, 16:", recalls)
    # the iteration cap is the same in all five runs: only the width differs
    assert any(set(a) != set(b) for a, b in zip(found[1], found[16]))
    assert all(b >= a for a, b in zip(recalls, recalls[1:])), recalls
    assert recalls[-1] > recalls[0], recalls


@pytest.mark.parametrize(
    "n,params",
    [
        (2000, {"graph_degree": 16, "itopk_size": 64, "max_iterations": 8}),
        (3000, {"graph_degree": 32, "itopk_size": 128, "max_iterations": 10}),
    ],
)
def test_specified_search_recall_is_not_below_the_torch_search(n, params):
    """Pins the specification: on the project's own graph, with each shape's
    default search_width, the model's recall@10 is at least the torch beam
    search's minus 0.01 (measured 0.9970 vs 0.9720 and 0.9990 vs 0.9960)."""
    X = _data(n, 16)
    Q = X[:100]
    k = 10
    truth = brute_force(Q, X, k)
    itopk, width, max_it = knn._cagra_search_params(params, k)
    assert width == max(4, itopk // 8)
    index = knn._cagra_build(torch.from_numpy(X), params)
    assert index.G.dtype == torch.int32
    assert index.G.shape == (n, params["graph_degree"] * 3 // 2)
    _, t_ids = knn._graph_beam_search(
        torch.from_numpy(Q), index.Xt, index.G.long(), k, itopk, max_it, expand=width
    )
    g = torch.Generator(device="cpu")
    g.manual_seed(11)
    seeds = torch.randint(0, n, (Q.shape[0], itopk), generator=g).numpy()
    G = index.G.numpy()
    m_ids = np.stack(
        [cagra_search_model(Q[i], X, G, seeds[i], k, itopk, width, max_it)[1]
         for i in range(Q.shape[0])]
    )
    r_torch, r_model = recall(t_ids.numpy(), truth), recall(m_ids, truth)
    print(f"n={n}: recall@10 torch {r_torch:.4f}, specified search {r_model:.4f}")
    assert r_model >= r_torch - 0.01


def test_ivfflat_keeps_its_coarse_index(monkeypatch):
    monkeypatch.delenv("SRML_ANN_CACHE", raising=False)
    calls = []
    real = knn._build_coarse

    def spy(*args, **kwargs):
        calls.append(1)
        return real(*args, **kwargs)

    monkeypatch.setattr(knn, "_build_coarse", spy)
    X = _data(1500, 8)
    Q = X[:20]
    model = ApproximateNearestNeighbors(
        k=5, algorithm="ivfflat", algoParams={"nlist": 16, "nprobe": 4}
    ).fit(DataFrame.from_numpy(X))
    first = _indices(model, Q)
    second = _indices(model, Q)
    assert len(calls) == 1
    np.testing.assert_array_equal(first[0], second[0])
    np.testing.assert_array_equal(first[1], second[1])
    # nprobe is a search parameter; nlist rebuilds
    model._set_params(algoParams={"nlist": 16, "nprobe": 8})
    _indices(model, Q)
    assert len(calls) == 1
    model._set_params(algoParams={"nlist": 8, "nprobe": 4})
    _indices(model, Q)
    assert len(calls) == 2
