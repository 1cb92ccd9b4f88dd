"""CAGRA's optimised build on the CPU: a plain numpy model of the rank-based
pruning and of the reverse-edge merge (tests/test_cagra_prune_gpu.py imports
it and compares the `cagra_prune` kernel to it), the torch formulations
against that model, and the `intermediate_graph_degree` / `build_algo`
algoParams at the model level."""

import warnings

import numpy as np
import pytest
import torch

from spark_rapids_ml_amd import ApproximateNearestNeighbors
from spark_rapids_ml_amd.data import DataFrame
from spark_rapids_ml_amd.models import knn
from tests.test_cagra import brute_force, recall


# -- the model ---------------------------------------------------------------------
def prune_model(G, d_out):
    """(P [n, d_out] i64, detour [n, D] i32) by the definition. Membership in
    a neighbour's raw row is read off a dense n x n adjacency matrix."""
    G = np.asarray(G, dtype=np.int64)
    n, D = G.shape
    live = np.zeros((n, D), dtype=bool)
    for u in range(n):
        seen = set()
        for j, v in enumerate(G[u].tolist()):
            live[u, j] = v != u and v not in seen
            seen.add(v)
    adj = np.zeros((n, n), dtype=bool)
    adj[np.arange(n)[:, None], G] = True
    member = adj[G[:, :, None], G[:, None, :]]  # [u, i, j]: G[u][j] in row of G[u][i]
    earlier = np.triu(np.ones((D, D), dtype=bool), 1)  # i < j
    detour = (member & live[:, :, None] & earlier[None]).sum(axis=1).astype(np.int32)
    detour[~live] = -1
    P = np.empty((n, d_out), dtype=np.int64)
    for u in range(n):
        ranked = sorted((int(detour[u, j]), j) for j in range(D) if live[u, j])
        row = [int(G[u, j]) for _, j in ranked[:d_out]]
        P[u] = row + [u] * (d_out - len(row))
    return P, detour


def merge_model(P):
    """F [n, d_out] i64 by the definition, with plain loops."""
    P = np.asarray(P, dtype=np.int64)
    n, d_out = P.shape
    h = d_out // 2
    rev = [[] for _ in range(n)]
    for k in range(d_out):
        for u in range(n):
            v = int(P[u, k])
            if v != u and len(rev[v]) < d_out:
                rev[v].append(u)
    F = np.empty((n, d_out), dtype=np.int64)
    for u in range(n):
        out = []
        for v in P[u, :h].tolist() + rev[u] + P[u, h:].tolist():
            if v != u and v not in out:
                out.append(v)
        out = out[:d_out]
        F[u] = out + [u] * (d_out - len(out))
    return F


# -- integer graphs ----------------------------------------------------------------
def distinct_rows(n, D, seed):
    """Every row: D distinct ids other than the row's own, in random order."""
    rng = np.random.default_rng(seed)
    G = np.empty((n, D), dtype=np.int64)
    for u in range(n):
        others = rng.permutation(n - 1)[:D]
        G[u] = others + (others >= u)
    return G


def ring(n, D):
    return (np.arange(n)[:, None] + 1 + np.arange(D)[None, :]) % n


def any_ids(n, D, seed):
    """Ids drawn from [0, n) with replacement: repeats and self-loops."""
    return np.random.default_rng(seed).integers(0, n, size=(n, D))


def congruent_rows(n, D, modulus, seed):
    """Every id of row u is congruent to u modulo `modulus`."""
    rng = np.random.default_rng(seed)
    steps = rng.integers(0, n // modulus, size=(n, D))
    return np.arange(n)[:, None] % modulus + modulus * steps


SHORT_ROWS = dict(n=40, D=64, d_out=32, seed=0)  # some rows keep < d_out live entries


def prune_cases():
    """name -> (G, d_out): the cases both the torch path and the kernel run."""
    s = SHORT_ROWS
    return {
        "distinct_24_to_8": (distinct_rows(300, 24, 1), 8),
        "one_to_one": (distinct_rows(50, 1, 2), 1),
        "two_to_one": (distinct_rows(50, 2, 3), 1),
        "keep_all_24": (distinct_rows(300, 24, 4), 24),
        "ring_500_16": (ring(500, 16), 8),
        "clique_17": (ring(17, 16), 8),
        "short_rows": (any_ids(s["n"], s["D"], s["seed"]), s["d_out"]),
    }


_WANT = {}


def prune_want(name):
    """The model's answer for a case of `prune_cases`, computed once."""
    if name not in _WANT:
        G, d_out = prune_cases()[name]
        _WANT[name] = (G, d_out) + prune_model(G, d_out)
    return _WANT[name]


# -- the model itself, where the answer is known -----------------------------------
@pytest.mark.parametrize("name", ["ring_500_16", "clique_17"])
def test_model_on_the_ring(name):
    G, d_out, P, detour = prune_want(name)
    D = G.shape[1]
    np.testing.assert_array_equal(detour, np.tile(np.arange(D), (G.shape[0], 1)))
    np.testing.assert_array_equal(P, G[:, :d_out])


def test_short_rows_have_fewer_live_entries_than_d_out():
    G, d_out, P, detour = prune_want("short_rows")
    n_live = (detour >= 0).sum(axis=1)
    assert (n_live < d_out).any() and (n_live >= d_out).any(), n_live
    own = np.arange(G.shape[0])[:, None]
    assert ((P == own).sum(axis=1) == np.maximum(0, d_out - n_live)).all()
    assert (G == own).any()  # self-loops are among the dead entries


# -- torch path against the model --------------------------------------------------
@pytest.mark.parametrize("name", sorted(prune_cases()))
def test_torch_prune_equals_the_model(name, monkeypatch):
    monkeypatch.delenv("SRML_CAGRA_PRUNE_KERNEL", raising=False)
    G, d_out, want_P, want_detour = prune_want(name)
    P, detour = knn._cagra_prune(torch.from_numpy(G), d_out)
    assert detour.dtype == torch.int32 and tuple(P.shape) == (G.shape[0], d_out)
    np.testing.assert_array_equal(detour.numpy(), want_detour)
    np.testing.assert_array_equal(P.numpy(), want_P)


def test_torch_prune_is_the_same_in_small_row_chunks(monkeypatch):
    G, d_out, want_P, want_detour = prune_want("distinct_24_to_8")
    monkeypatch.setattr(knn, "_CAGRA_PRUNE_CHUNK_ELEMS", 1 << 12)  # 7 rows per chunk at D = 24
    P, detour = knn._cagra_prune(torch.from_numpy(G.astype(np.int32)), d_out)  # i32 in as well
    np.testing.assert_array_equal(detour.numpy(), want_detour)
    np.testing.assert_array_equal(P.numpy(), want_P)


def test_prune_rejects_a_bad_d_out():
    G = torch.from_numpy(distinct_rows(20, 4, 0))
    for bad in (0, 5):
        with pytest.raises(ValueError, match="D_out"):
            knn._cagra_prune(G, bad)


def _merge_special():
    """n = 60, 4 columns: node 0 is a hub that 54 rows point at first, node 59
    is pointed at by nobody, rows 50..54 are all filler."""
    rng = np.random.default_rng(5)
    n, d_out = 60, 4
    P = np.empty((n, d_out), dtype=np.int64)
    for u in range(n):
        others = [v for v in rng.permutation(np.arange(1, 59)).tolist() if v != u][: d_out - 1]
        P[u] = [0] + others if u != 0 else others + [u]
    P[50:55] = np.arange(50, 55)[:, None]
    return P


def test_merge_reverse_equals_the_model():
    P = _merge_special()
    assert not (P == 59).any()
    assert ((P == 0).sum() - (P[0] == 0).sum()) > P.shape[1]
    assert (P[50:55] == np.arange(50, 55)[:, None]).all()
    F = knn._cagra_merge_reverse(torch.from_numpy(P)).numpy()
    want = merge_model(P)
    np.testing.assert_array_equal(F, want)
    assert list(F[59]) == list(P[59])  # no reverse edge to merge
    # an all-filler row holds reverse edges only
    rev_52 = {u for u in range(60) if 52 in P[u] and u != 52}
    assert set(F[52]) - {52} <= rev_52


@pytest.mark.parametrize("name", ["distinct_24_to_8", "short_rows", "one_to_one", "ring_500_16"])
def test_merge_reverse_equals_the_model_on_pruned_graphs(name):
    _, _, P, _ = prune_want(name)
    F = knn._cagra_merge_reverse(torch.from_numpy(P)).numpy()
    np.testing.assert_array_equal(F, merge_model(P))
    own = np.arange(P.shape[0])[:, None]
    for row, u in zip(F, own[:, 0]):  # distinct apart from the filler
        real = row[row != u]
        assert len(set(real.tolist())) == len(real)


# -- model level -------------------------------------------------------------------
def _data(n, d, seed=0):
    return np.random.default_rng(seed).normal(size=(n, d)).astype(np.float32)


def _fit(X, k, params):
    return ApproximateNearestNeighbors(k=k, algorithm="cagra", algoParams=params).fit(
        DataFrame.from_numpy(X)
    )


def _indices(model, Q):
    _, _, res = model.kneighbors(DataFrame.from_numpy(Q))
    return np.asarray(res["indices"]), np.asarray(res["distances"])


@pytest.fixture
def build_calls(monkeypatch):
    """Degrees `_nn_descent` was asked for, and (degree, build_algo) of every
    intermediate graph."""
    calls = {"nn_descent": [], "knn_graph": []}
    real_nd, real_kg = knn._nn_descent, knn._cagra_knn_graph

    def spy_nd(X, degree, n_iter):
        calls["nn_descent"].append(degree)
        return real_nd(X, degree, n_iter)

    def spy_kg(Xt, degree, build_algo, n_iter):
        calls["knn_graph"].append((degree, build_algo))
        return real_kg(Xt, degree, build_algo, n_iter)

    monkeypatch.setattr(knn, "_nn_descent", spy_nd)
    monkeypatch.setattr(knn, "_cagra_knn_graph", spy_kg)
    return calls


OPT = {"graph_degree": 32, "intermediate_graph_degree": 64}


def test_optimised_graph_has_exactly_graph_degree_columns(build_calls, monkeypatch):
    monkeypatch.delenv("SRML_ANN_CACHE", raising=False)
    X = _data(2000, 16)
    Q = X[:20]
    model = _fit(X, 10, dict(OPT))
    first = _indices(model, Q)
    G = model._ann_index[1].G
    assert G.dtype == torch.int32 and tuple(G.shape) == (2000, 32) and G.is_contiguous()
    assert build_calls["nn_descent"] == [64]
    second = _indices(model, Q)
    assert build_calls["nn_descent"] == [64]  # the kept index
    np.testing.assert_array_equal(first[0], second[0])
    # a search parameter does not rebuild
    model._set_params(algoParams={**OPT, "itopk_size": 96})
    _indices(model, Q)
    assert build_calls["knn_graph"] == [(64, "nn_descent")]
    # naming the default build_algo resolves to the same index
    model._set_params(algoParams={**OPT, "build_algo": "nn_descent"})
    _indices(model, Q)
    assert build_calls["knn_graph"] == [(64, "nn_descent")]
    # either build parameter rebuilds
    model._set_params(algoParams={**OPT, "intermediate_graph_degree": 48})
    _indices(model, Q)
    assert build_calls["knn_graph"] == [(64, "nn_descent"), (48, "nn_descent")]
    assert tuple(model._ann_index[1].G.shape) == (2000, 32)
    model._set_params(algoParams={**OPT, "intermediate_graph_degree": 48, "build_algo": "ivf_pq"})
    idx, dist = _indices(model, Q)
    assert build_calls["knn_graph"][-1] == (48, "ivf_pq") and len(build_calls["knn_graph"]) == 3
    assert build_calls["nn_descent"] == [64, 48]
    assert ((idx >= 0) & (idx < 2000)).all() and np.isfinite(dist).all()


def test_without_the_new_parameters_the_build_is_unchanged(build_calls):
    X = _data(600, 8)
    model = _fit(X, 5, {"graph_degree": 16})
    _indices(model, X[:5])
    assert build_calls["knn_graph"] == [] and build_calls["nn_descent"] == [16]
    assert tuple(model._ann_index[1].G.shape) == (600, 24)
    key_names = [name for name, _ in model._ann_index[0][1]]
    assert key_names == ["graph_degree", "nn_descent_niter"]


def test_optimised_graph_searches_no_worse_than_truncation(monkeypatch):
    """Same intermediate graph, same search (itopk 64, width 1, 20
    iterations, torch search): the pruned and merged 32 columns against the
    plain first 32. Measured 0.952 against 0.880; the order is asserted."""
    monkeypatch.setenv("SRML_CAGRA_KERNEL", "0")
    X = _data(2000, 16)
    Q = X[:500]
    truth = brute_force(Q, X, 10)
    search = {"itopk_size": 64, "search_width": 1, "max_iterations": 20}
    model = _fit(X, 10, {**OPT, **search})
    r_opt = recall(_indices(model, Q)[0], truth)
    Xt = torch.from_numpy(X)
    G64 = knn._nn_descent(Xt, 64, 3)
    np.testing.assert_array_equal(
        model._ann_index[1].G.numpy(), knn._cagra_optimize(G64, 32).numpy()
    )
    plain = knn.CagraIndex(Xt=Xt, G=G64[:, :32].to(torch.int32).contiguous())
    _, ids = knn._cagra_query(plain, torch.from_numpy(Q), 10, 64, 1, 20)
    r_plain = recall(ids.numpy(), truth)
    print(f"recall@10: optimised 64->32 {r_opt:.4f}, forward top-32 {r_plain:.4f}")
    assert r_opt >= r_plain


# -- parameters --------------------------------------------------------------------
def test_graph_degree_above_the_intermediate_degree_is_lowered():
    with pytest.warns(RuntimeWarning, match="graph_degree"):
        got = knn._cagra_optimize_params(
            {"graph_degree": 48, "intermediate_graph_degree": 24}, 600
        )
    assert got == (24, 24, "nn_descent")
    X = _data(600, 8)
    model = _fit(X, 5, {"graph_degree": 48, "intermediate_graph_degree": 24})
    with pytest.warns(RuntimeWarning, match="graph_degree"):
        _indices(model, X[:5])
    assert tuple(model._ann_index[1].G.shape) == (600, 24)


def test_intermediate_degree_is_lowered_below_the_item_count():
    with pytest.warns(RuntimeWarning, match="intermediate_graph_degree") as caught:
        got = knn._cagra_optimize_params(
            {"graph_degree": 48, "intermediate_graph_degree": 64}, 40
        )
    assert got == (39, 39, "nn_descent")
    assert len([w for w in caught if issubclass(w.category, RuntimeWarning)]) == 2
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # in range: no warning, and the defaults
        assert knn._cagra_optimize_params({"build_algo": "nn_descent"}, 1000) == (
            32, 64, "nn_descent")
        assert knn._cagra_optimize_params({"graph_degree": 16}, 1000) is None
    X = _data(40, 8)
    model = _fit(X, 5, {"graph_degree": 16, "intermediate_graph_degree": 64})
    with pytest.warns(RuntimeWarning, match="intermediate_graph_degree"):
        idx, _ = _indices(model, X[:5])
    assert tuple(model._ann_index[1].G.shape) == (40, 16)
    assert ((idx >= 0) & (idx < 40)).all()


def test_unknown_build_algo_raises(build_calls):
    X = _data(100, 8)
    model = _fit(X, 5, {"build_algo": "hnsw"})
    with pytest.raises(ValueError, match="build_algo"):
        model.kneighbors(DataFrame.from_numpy(X[:4]))
    assert build_calls["knn_graph"] == []


def test_ivf_pq_rejects_an_intermediate_degree_of_256(build_calls):
    X = _data(100, 8)
    model = _fit(X, 5, {"build_algo": "ivf_pq", "intermediate_graph_degree": 256})
    with pytest.raises(
        ValueError,
        match=r"cagra with ivf_pq build_algo expects intermediate_graph_degree \(256\) "
        "to be smaller than 256",
    ):
        model.kneighbors(DataFrame.from_numpy(X[:4]))
    assert build_calls["knn_graph"] == []
    # nn_descent takes it
    assert knn._cagra_optimize_params(
        {"graph_degree": 64, "intermediate_graph_degree": 256}, 1000
    ) == (64, 256, "nn_descent")


# -- ivf_pq build ------------------------------------------------------------------
def test_ivf_pq_intermediate_graph():
    """Measured on the CPU: recall 0.919 against the exact kNN graph; the
    bound leaves 0.07 for another k-means course on another device."""
    n, D = 2000, 64
    X = _data(n, 16)
    G = knn._ivfpq_knn_graph(torch.from_numpy(X), D).numpy()
    assert G.shape == (n, D)
    own = np.arange(n)[:, None]
    assert ((G >= 0) & (G < n)).all()
    X64 = X.astype(np.float64)
    d2 = ((X64[:, None, :] - X64[None]) ** 2).sum(2)
    gd = np.take_along_axis(d2, G, axis=1)
    # the refine orders by f32 keys: 16 squares summed, each step within eps32
    tol = 32 * np.finfo(np.float32).eps * d2.max()
    hits = 0
    np.fill_diagonal(d2, np.inf)
    truth = np.argsort(d2, axis=1, kind="stable")[:, :D]
    for u in range(n):
        live = G[u] != u
        ids = G[u][live]
        assert len(set(ids.tolist())) == len(ids)
        assert (np.diff(gd[u][live]) >= -tol).all(), u
        hits += len(set(ids.tolist()) & set(truth[u].tolist()))
    graph_recall = hits / truth.size
    print(f"ivf_pq intermediate graph recall@{D}: {graph_recall:.4f}")
    assert graph_recall >= 0.85


def test_ivf_pq_build_end_to_end():
    X = _data(2000, 16)
    Q = X[:50]
    model = _fit(X, 10, {**OPT, "build_algo": "ivf_pq"})
    idx, dist = _indices(model, Q)
    assert tuple(model._ann_index[1].G.shape) == (2000, 32)
    assert ((idx >= 0) & (idx < 2000)).all() and np.isfinite(dist).all()
