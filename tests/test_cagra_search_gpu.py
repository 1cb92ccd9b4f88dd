"""GPU: the fused `cagra_search` kernel on exact-integer data (coordinates in
[-8, 8], so every key is exact in f32) against numpy float64 brute force and
the plain-Python model of tests/test_cagra.py, its host-side argument checks,
and cagra end to end on the device through the kernel."""

import numpy as np
import pytest
import torch

from spark_rapids_ml_amd import ApproximateNearestNeighbors
from spark_rapids_ml_amd.data import DataFrame
from spark_rapids_ml_amd.models import knn as knn_mod
from tests.test_cagra import brute_force, cagra_search_model, recall

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ext():
    from spark_rapids_ml_amd.ops.dispatch import hip_ops

    return hip_ops()


def _int_data(n, d, seed):
    return np.random.default_rng(seed).integers(-8, 9, size=(n, d)).astype(np.float32)


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _run(ext, Q, X, G, seeds, k, itopk, width, max_it, hash_bits=0):
    keys, ids, stats = ext.cagra_search(
        _f32(Q), _f32(X), _i32(G), _i32(seeds), k, itopk, width, max_it, hash_bits
    )
    torch.cuda.synchronize()
    return keys.cpu().numpy(), ids.cpu().numpy().astype(np.int64), stats.cpu().numpy()


def _exact_topk(Q, X, k):
    """float64 brute force in stable order, padded with (+inf, -1) past n."""
    n = X.shape[0]
    d2 = ((Q[:, None, :].astype(np.float64) - X[None].astype(np.float64)) ** 2).sum(2)
    order = np.argsort(d2, axis=1, kind="stable")[:, :k]
    keys = np.full((Q.shape[0], k), np.inf, dtype=np.float32)
    ids = np.full((Q.shape[0], k), -1, dtype=np.int64)
    m = min(k, n)
    keys[:, :m] = np.take_along_axis(d2, order, axis=1)[:, :m]
    ids[:, :m] = order[:, :m]
    return keys, ids


def _ring(n, steps):
    i = np.arange(n)[:, None]
    return (i + np.asarray(steps)[None, :]) % n


# -- exact limit: the whole ring is reached, every node keyed once -------------
@pytest.mark.parametrize(
    "d,k", [(7, 10), (1, 10), (64, 10), (65, 10), (300, 10), (7, 1), (7, 512)]
)
def test_exact_limit_fixes_order_and_stats(ext, d, k):
    n, nq = 500, 6
    X = _int_data(n, d, seed=d)
    Q = _int_data(nq, d, seed=1000 + d)
    G = _ring(n, [1, -1, 0, 1])  # a ring with a self-loop and a duplicate
    seeds = np.tile(np.array([0, 0, -1, 5]), (nq, 1))
    keys, ids, stats = _run(ext, Q, X, G, seeds, k, 512, 1, 10000)
    want_keys, want_ids = _exact_topk(Q, X, k)
    np.testing.assert_array_equal(ids, want_ids)
    np.testing.assert_array_equal(keys, want_keys)
    assert (stats[:, 1] == n).all(), stats
    assert (stats[:, 2] == 0).all(), stats
    assert (stats[:, 0] == n).all(), stats  # width 1: one parent per iteration


# -- iteration cap ---------------------------------------------------------------
@pytest.mark.parametrize("t", [1, 3, 17])
def test_iteration_cap(ext, t):
    n, nq, d = 500, 5, 7
    X = _int_data(n, d, seed=3)
    Q = _int_data(nq, d, seed=4)
    G = _ring(n, [1, -1])
    start = np.array([0, 7, 250, 499, 123])
    seeds = np.full((nq, 4), -1)
    seeds[:, 0] = start
    keys, ids, stats = _run(ext, Q, X, G, seeds, 10, 64, 1, t)
    for q in range(nq):
        found = ids[q][ids[q] >= 0]
        assert len(found) == min(10, stats[q, 1])
        steps = np.minimum((found - start[q]) % n, (start[q] - found) % n)
        assert (steps <= t).all(), (q, found)
        assert np.isinf(keys[q][ids[q] < 0]).all()
    assert (stats[:, 0] <= t).all() and (stats[:, 0] >= 1).all(), stats
    assert (stats[:, 1] <= 1 + 2 * t).all(), stats


def test_search_stops_by_itself_and_pads(ext):
    n, nq, d = 5, 4, 7
    X = _int_data(n, d, seed=5)
    Q = _int_data(nq, d, seed=6)
    seeds = np.full((nq, 4), -1)
    seeds[:, 0] = [0, 1, 2, 4]
    keys, ids, stats = _run(ext, Q, X, _ring(n, [1, -1]), seeds, 8, 32, 1, 1000)
    want_keys, want_ids = _exact_topk(Q, X, 8)
    np.testing.assert_array_equal(ids, want_ids)
    np.testing.assert_array_equal(keys, want_keys)
    assert (ids[:, 5:] == -1).all() and np.isinf(keys[:, 5:]).all()
    assert (stats[:, 0] <= 5).all(), stats
    assert (stats[:, 1] == 5).all(), stats


# -- trimming against the Python model -------------------------------------------
_TRIM = {}


def _trim_case():
    if not _TRIM:
        n, d, nq, itopk = 2000, 7, 16, 64
        X = _int_data(n, d, seed=11)
        Q = _int_data(nq, d, seed=12)
        X64 = X.astype(np.float64)
        sq = (X64 * X64).sum(1)
        d2 = sq[:, None] + sq[None, :] - 2.0 * (X64 @ X64.T)  # exact: integers
        np.fill_diagonal(d2, np.inf)
        G = np.argsort(d2, axis=1, kind="stable")[:, :8]
        seeds = np.random.default_rng(13).integers(0, n, size=(nq, itopk))
        _TRIM.update(X=X, Q=Q, G=G, seeds=seeds, itopk=itopk, model={})
    return _TRIM


def _trim_model(width, max_it):
    c = _trim_case()
    if (width, max_it) not in c["model"]:
        rows = [
            cagra_search_model(c["Q"][i], c["X"], c["G"], c["seeds"][i], 64, c["itopk"],
                               width, max_it)
            for i in range(c["Q"].shape[0])
        ]
        c["model"][(width, max_it)] = (
            np.stack([r[0] for r in rows]),
            np.stack([r[1] for r in rows]),
            np.array([r[2] for r in rows]),
        )
    return c["model"][(width, max_it)]


@pytest.mark.parametrize("max_it", [3, 40])
@pytest.mark.parametrize("width", [1, 4, 8])
@pytest.mark.parametrize("k", [1, 10, 64])
def test_trimming_matches_the_python_model(ext, k, width, max_it):
    c = _trim_case()
    want_keys, want_ids, want_stats = _trim_model(width, max_it)
    keys, ids, stats = _run(ext, c["Q"], c["X"], c["G"], c["seeds"], k, c["itopk"], width, max_it)
    np.testing.assert_array_equal(ids, want_ids[:, :k])
    np.testing.assert_array_equal(keys, want_keys[:, :k])
    np.testing.assert_array_equal(stats[:, 0], want_stats[:, 0])
    # hash_bits = 0 at n = 2000 gives a filter that never resets
    assert (stats[:, 2] == 0).all()
    np.testing.assert_array_equal(stats[:, 1], want_stats[:, 1])


def test_filter_resets_change_only_the_stats(ext):
    c = _trim_case()
    args = (c["Q"], c["X"], c["G"], c["seeds"], 64, c["itopk"], 4, 40)
    # minimum table: 2 * (itopk + search_width * deg) = 192 slots -> 2**8
    keys_s, ids_s, stats_s = _run(ext, *args, hash_bits=8)
    keys_l, ids_l, stats_l = _run(ext, *args, hash_bits=12)
    np.testing.assert_array_equal(ids_s, ids_l)
    np.testing.assert_array_equal(keys_s, keys_l)
    np.testing.assert_array_equal(stats_s[:, 0], stats_l[:, 0])
    assert (stats_s[:, 2] > 0).all(), stats_s
    assert (stats_l[:, 2] == 0).all(), stats_l
    assert (stats_s[:, 1] >= stats_l[:, 1]).all()
    want_keys, want_ids, want_stats = _trim_model(4, 40)
    np.testing.assert_array_equal(ids_s, want_ids)
    np.testing.assert_array_equal(stats_l[:, 1], want_stats[:, 1])


# -- wrapper ----------------------------------------------------------------------
def _wargs(n=64, d=8, deg=8, nq=3, ns=16):
    rng = np.random.default_rng(0)
    return [
        _f32(_int_data(nq, d, 1)),
        _f32(_int_data(n, d, 2)),
        _i32(rng.integers(0, n, size=(n, deg))),
        _i32(rng.integers(0, n, size=(nq, ns))),
    ]


def test_wrapper_rejects_bad_arguments(ext):
    keys, ids, stats = ext.cagra_search(*_wargs(), 4, 32, 2, 5, 0)  # accepted
    assert keys.shape == (3, 4) and ids.dtype == torch.int32 and stats.shape == (3, 3)
    a = _wargs()
    a[0] = a[0].double()
    with pytest.raises(RuntimeError, match="Q and X"):
        ext.cagra_search(*a, 4, 32, 2, 5, 0)  # Q not f32
    a = _wargs()
    a[2] = a[2].long()
    with pytest.raises(RuntimeError, match="G and seeds"):
        ext.cagra_search(*a, 4, 32, 2, 5, 0)  # G not i32
    a = _wargs()
    a[1] = a[1].t().contiguous().t()
    with pytest.raises(RuntimeError, match="Q and X"):
        ext.cagra_search(*a, 4, 32, 2, 5, 0)  # X not contiguous
    a = _wargs()
    a[3] = a[3].cpu()
    with pytest.raises(RuntimeError, match="G and seeds"):
        ext.cagra_search(*a, 4, 32, 2, 5, 0)  # seeds on the host
    with pytest.raises(RuntimeError, match="k <= itopk"):
        ext.cagra_search(*_wargs(), 0, 32, 2, 5, 0)  # k = 0
    with pytest.raises(RuntimeError, match="k <= itopk"):
        ext.cagra_search(*_wargs(), 33, 32, 2, 5, 0)  # k > itopk
    with pytest.raises(RuntimeError, match="itopk <= 512"):
        ext.cagra_search(*_wargs(), 4, 513, 2, 5, 0)  # itopk = 513
    ext.cagra_search(*_wargs(), 512, 512, 2, 5, 0)  # itopk = k = 512 is the boundary
    with pytest.raises(RuntimeError, match="d <= 2048"):
        ext.cagra_search(*_wargs(d=2049), 4, 32, 2, 5, 0)  # d = 2049
    ext.cagra_search(*_wargs(d=2048), 4, 32, 2, 5, 0)
    with pytest.raises(RuntimeError, match="deg <= 128"):
        ext.cagra_search(*_wargs(deg=129), 4, 32, 2, 5, 0)  # deg = 129
    ext.cagra_search(*_wargs(deg=128), 4, 32, 2, 5, 0)
    with pytest.raises(RuntimeError, match="search_width"):
        ext.cagra_search(*_wargs(), 4, 32, 0, 5, 0)  # search_width = 0
    with pytest.raises(RuntimeError, match="search_width"):
        ext.cagra_search(*_wargs(), 4, 32, 257, 5, 0)  # search_width * deg = 2056
    ext.cagra_search(*_wargs(), 4, 32, 256, 5, 0)  # = 2048
    with pytest.raises(RuntimeError, match="max_iterations"):
        ext.cagra_search(*_wargs(), 4, 32, 2, 0, 0)  # max_iterations = 0
    a = _wargs()
    a[3] = a[3][:2].contiguous()
    with pytest.raises(RuntimeError, match="row count"):
        ext.cagra_search(*a, 4, 32, 2, 5, 0)  # seeds and Q differ in row count
    with pytest.raises(RuntimeError, match="seeds per query"):
        ext.cagra_search(*_wargs(ns=2049), 4, 32, 2, 5, 0)  # 2049 seeds per query
    ext.cagra_search(*_wargs(ns=2048), 4, 32, 2, 5, 0)
    # minimum filter: 2 * (32 + 2 * 8) = 96 slots -> hash_bits 7
    with pytest.raises(RuntimeError, match="hash_bits"):
        ext.cagra_search(*_wargs(), 4, 32, 2, 5, 6)
    ext.cagra_search(*_wargs(), 4, 32, 2, 5, 7)
    with pytest.raises(RuntimeError, match="LDS"):
        ext.cagra_search(*_wargs(), 4, 32, 2, 5, 16)  # a 256 KiB filter
    a = _wargs(d=1)
    a[1] = torch.empty((2**31, 1), dtype=torch.float32, device="cuda")  # never read
    with pytest.raises(RuntimeError, match="n < 2\\*\\*31"):
        ext.cagra_search(*a, 4, 32, 2, 5, 0)  # n = 2**31
    torch.cuda.synchronize()


# -- model level ------------------------------------------------------------------
def _spy_on_op(monkeypatch, ext):
    calls = []
    real = ext.cagra_search

    def spy(*a, **kw):
        calls.append(a[4:])  # (k, itopk, search_width, max_iterations, hash_bits)
        return real(*a, **kw)

    monkeypatch.setattr(ext, "cagra_search", spy)
    return calls


def _neighbors(model, Q):
    _, _, res = model.kneighbors(DataFrame.from_numpy(Q))
    return np.asarray(res["indices"]), np.asarray(res["distances"])


def test_cagra_searches_with_the_kernel_on_the_device(monkeypatch, ext):
    monkeypatch.delenv("SRML_CAGRA_KERNEL", raising=False)
    monkeypatch.delenv("SRML_ANN_CACHE", raising=False)
    calls = _spy_on_op(monkeypatch, ext)
    X = np.random.default_rng(0).normal(size=(3000, 16)).astype(np.float32)
    Q = X[:100]
    params = {"graph_degree": 32, "itopk_size": 128, "max_iterations": 10}
    model = ApproximateNearestNeighbors(k=10, algorithm="cagra", algoParams=params).fit(
        DataFrame.from_numpy(X)
    )
    idx_k, dist_k = _neighbors(model, Q)
    assert len(calls) == 1, "cagra searches with the cagra_search kernel on the device"
    idx_2, dist_2 = _neighbors(model, Q)  # the kept index, same arrays
    np.testing.assert_array_equal(idx_k, idx_2)
    np.testing.assert_array_equal(dist_k, dist_2)
    monkeypatch.setenv("SRML_CAGRA_KERNEL", "0")
    n_calls = len(calls)
    idx_t, _ = _neighbors(model, Q)  # torch search on the same kept graph
    assert len(calls) == n_calls
    truth = brute_force(Q, X, 10)
    r_kernel, r_torch = recall(idx_k, truth), recall(idx_t, truth)
    print(f"recall@10: kernel {r_kernel:.4f}, torch {r_torch:.4f}")
    assert r_kernel >= r_torch - 0.01
    true_d = np.sqrt(
        ((Q[:, None, :].astype(np.float64) - X[idx_k].astype(np.float64)) ** 2).sum(2)
    )
    np.testing.assert_allclose(dist_k, true_d, rtol=1e-4, atol=1e-4)


def test_search_width_reaches_the_kernel(monkeypatch, ext):
    monkeypatch.delenv("SRML_CAGRA_KERNEL", raising=False)
    calls = _spy_on_op(monkeypatch, ext)
    X = np.random.default_rng(0).normal(size=(2000, 16)).astype(np.float32)
    Q = X[:100]
    truth = brute_force(Q, X, 10)
    base = {"graph_degree": 16, "itopk_size": 64, "max_iterations": 8}
    model = ApproximateNearestNeighbors(k=10, algorithm="cagra", algoParams=base).fit(
        DataFrame.from_numpy(X)
    )
    found = {}
    for width in (None, 1, 16):
        params = dict(base) if width is None else {**base, "search_width": width}
        model._set_params(algoParams=params)
        found[width] = _neighbors(model, Q)[0]
    assert [c[:4] for c in calls] == [(10, 64, 8, 8), (10, 64, 1, 8), (10, 64, 16, 8)]
    assert any(set(a) != set(b) for a, b in zip(found[1], found[16]))
    r1, r16 = recall(found[1], truth), recall(found[16], truth)
    print(f"recall@10: search_width 1 {r1:.4f}, 16 {r16:.4f}")
    assert r16 > r1


def test_fewer_items_than_k_pads(monkeypatch, ext):
    monkeypatch.delenv("SRML_CAGRA_KERNEL", raising=False)
    calls = _spy_on_op(monkeypatch, ext)
    X = np.random.default_rng(1).normal(size=(40, 8)).astype(np.float32)
    model = ApproximateNearestNeighbors(
        k=64, algorithm="cagra", algoParams={"graph_degree": 8}
    ).fit(DataFrame.from_numpy(X))
    idx, dist = _neighbors(model, X[:7])
    assert calls
    assert (idx[:, 40:] == -1).all() and np.isinf(dist[:, 40:]).all()
    assert (idx[:, :40] >= 0).all() and np.isfinite(dist[:, :40]).all()
    # the graph of 40 items is connected enough to reach all of them
    assert all(sorted(row[:40]) == list(range(40)) for row in idx)
