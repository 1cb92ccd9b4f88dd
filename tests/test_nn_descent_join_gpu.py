"""The `nn_descent_join` kernel (one nn-descent round per launch) against a
numpy reference, its dispatch from `_nn_descent`, and the recall of the graph.

Items are small integers in [-8, 8] held in f32: every squared distance is an
exact integer below 2**24, so the kernel must agree exactly with the int64
reference. Every check is invariant to how ties are broken."""

import numpy as np
import pytest
import torch

from spark_rapids_ml_amd import UMAP, ApproximateNearestNeighbors
from spark_rapids_ml_amd.data import DataFrame
from spark_rapids_ml_amd.models import knn

pytestmark = pytest.mark.gpu
FILL = np.float32(3.4e38)


@pytest.fixture(scope="module")
def ext():
    from spark_rapids_ml_amd.ops.dispatch import hip_ops

    return hip_ops()


def _sq_dists(X):
    Xd = X.astype(np.float64)
    sq = (Xd * Xd).sum(1)
    return (sq[:, None] + sq[None, :] - 2.0 * (Xd @ Xd.T)).astype(np.int64)


def _inputs(n, d, deg, variant=None, seed=0):
    """(X, D, G, Gd, join, rev): a random list with a repeat and own ids in it,
    its keys, and the joined lists `_nn_descent` would pick."""
    rng = np.random.default_rng(seed)
    X = rng.integers(-8, 9, size=(n, d)).astype(np.float32)
    D = _sq_dists(X)
    assert D.max() < 2 ** 24
    G = rng.integers(0, n, size=(n, deg), dtype=np.int64)
    G[:, 1] = G[:, 0]
    G[::3, deg // 2] = np.arange(n)[::3]
    if variant == "shared":  # one id in every list, so in every joined list
        G[:, 3] = 5
    Gt = torch.from_numpy(G).cuda()
    rev = knn._reverse_edges(Gt, min(deg, 8))
    if variant == "rev_filler":
        rev = torch.arange(n, device="cuda")[:, None].expand(n, min(deg, 8)).contiguous()
    join = torch.cat([Gt[:, : min(deg, 8)], rev], dim=1)
    Gd = torch.from_numpy(np.take_along_axis(D, G, 1).astype(np.float32)).cuda()
    return torch.from_numpy(X).cuda(), D, Gt, Gd, join, rev


def _check_round(D, G, join, rev, G_new, Gd_new):
    """Check 1 of the kernel's (G_new, Gd_new) against the candidate sets."""
    G, join, rev = G.cpu().numpy(), join.cpu().numpy(), rev.cpu().numpy()
    ids_all, keys_all = G_new.cpu().numpy(), Gd_new.cpu().numpy()
    deg = G.shape[1]
    assert ids_all.dtype == np.int64 and ids_all.shape == G.shape == keys_all.shape
    for i in range(G.shape[0]):
        cand = (set(G[i]) | set(G[join[i]].ravel()) | set(rev[i])) - {i}
        want = np.sort(D[i, sorted(cand)])[:deg]
        ids, keys = ids_all[i], keys_all[i]
        real = np.arange(deg) < len(want)
        assert len(set(ids[real])) == len(want) and set(ids[real]) <= cand, i
        named = D[i, ids[real]]
        np.testing.assert_array_equal(np.sort(named), want, err_msg=str(i))
        np.testing.assert_array_equal(keys[real], named.astype(np.float32), err_msg=str(i))
        assert (np.diff(keys) >= 0).all(), i
        assert (ids[~real] == i).all() and (keys[~real] == FILL).all(), i


CASES = [
    # n, d, deg, variant
    (700, 8, 32, None),          # ordinary
    (300, 3, 32, None),          # partial first segment, four teams per wave
    (300, 32, 32, None),         # teams, both elements of every lane
    (300, 64, 32, None),
    (300, 65, 32, None),         # second segment
    (300, 200, 32, None),        # wider rows
    (300, 300, 32, None),        # two rows in flight
    (200, 600, 32, None),        # one row in flight
    (300, 8, 8, None),           # J = 16
    (300, 8, 64, None),
    (300, 8, 65, None),          # one lane-slot past
    (300, 8, 128, None),
    (400, 8, 256, None),         # the cap
    (34, 8, 32, None),           # n = deg + 2: nearly every row short
    (300, 8, 32, "rev_filler"),
    (300, 8, 32, "shared"),
]


@pytest.mark.parametrize("n,d,deg,variant", CASES)
def test_one_round_matches_the_reference(n, d, deg, variant):
    X, D, G, Gd, join, rev = _inputs(n, d, deg, variant)
    G_new, Gd_new = knn._nnd_step_kernel(X, G, Gd, join, rev)
    _check_round(D, G, join, rev, G_new, Gd_new)


def test_three_chained_rounds():
    X, D, G, Gd, _, _ = _inputs(700, 8, 32)
    for _ in range(3):
        rev = knn._reverse_edges(G, 8)
        join = torch.cat([G[:, :8], rev], dim=1)
        stats = torch.zeros(700, dtype=torch.int32, device="cuda")
        G_new, Gd_new = knn._nnd_step_kernel(X, G, Gd, join, rev, stats)
        _check_round(D, G, join, rev, G_new, Gd_new)
        # rows were skipped, not all of the 16 * 32 + 8 candidates keyed
        assert 0 < stats.float().mean().item() < join.shape[1] * 32 + rev.shape[1]
        G, Gd = knn._nnd_step_torch(X, G, Gd, join, rev)


def _boom(*args, **kwargs):
    raise AssertionError("this path must not run")


def _items(n=600, d=8):
    return np.random.default_rng(0).normal(size=(n, d)).astype(np.float32)


def test_public_paths_take_the_kernel(monkeypatch):
    monkeypatch.delenv("SRML_NND_KERNEL", raising=False)
    monkeypatch.setattr(knn, "_nnd_step_torch", _boom)
    df = DataFrame.from_numpy(_items())
    model = ApproximateNearestNeighbors(k=5, algorithm="cagra").fit(df)
    _, _, res = model.kneighbors(DataFrame.from_numpy(_items()[:10]))
    assert np.asarray(res["indices"]).shape == (10, 5)
    UMAP(build_algo="nn_descent", n_neighbors=15, n_epochs=5).fit(df)


@pytest.mark.parametrize("env,degree", [("0", 32), (None, 257)])
def test_torch_step_when_forced_or_past_the_cap(ext, monkeypatch, env, degree):
    monkeypatch.delenv("SRML_NND_KERNEL", raising=False)
    if env is not None:
        monkeypatch.setenv("SRML_NND_KERNEL", env)
    monkeypatch.setattr(ext, "nn_descent_join", _boom)
    G = knn._nn_descent(torch.from_numpy(_items()).cuda(), degree, 1)
    assert G.shape == (600, degree) and G.dtype == torch.int64


def test_binding_limits(ext):
    X, _, G, Gd, join, rev = _inputs(300, 8, 32)
    with pytest.raises(RuntimeError, match="alias"):
        ext.nn_descent_join(X, G, Gd, join, rev, G, torch.empty_like(Gd))
    with pytest.raises(RuntimeError, match="alias"):
        ext.nn_descent_join(X, G, Gd, join, rev, torch.empty_like(G), Gd)
    Gw = torch.zeros((300, 257), dtype=torch.int64, device="cuda")
    Gdw = torch.zeros((300, 257), device="cuda")
    with pytest.raises(RuntimeError, match="deg <= 256"):
        ext.nn_descent_join(X, Gw, Gdw, join, rev, torch.empty_like(Gw), torch.empty_like(Gdw))


# Recall of the torch path alone on five row permutations of the same items
# (a different order changes tie and rounding outcomes as the kernel does),
# `tools/time_nn_descent.py --shapes recall --permutations 5` on the MI355X:
# 0.9527, 0.9537, 0.9562, 0.9534, 0.9527; max - min is the margin.
RECALL_MARGIN = 0.0035


def test_recall_not_below_the_torch_path(monkeypatch):
    X = _items(2000, 16)
    truth = np.argsort(_sq_dists_f64(X), axis=1, kind="stable")[:, 1:33]
    Xt = torch.from_numpy(X).cuda()
    got = {}
    for env in ("0", "1"):
        monkeypatch.setenv("SRML_NND_KERNEL", env)
        G = knn._nn_descent(Xt, 32, 3).cpu().numpy()
        got[env] = np.mean([len(set(g) & set(t)) / 32 for g, t in zip(G, truth)])
    print(f"recall: torch {got['0']:.4f}, kernel {got['1']:.4f}")
    assert got["1"] >= got["0"] - RECALL_MARGIN


def _sq_dists_f64(X):
    Xd = X.astype(np.float64)
    sq = (Xd * Xd).sum(1)
    return sq[:, None] + sq[None, :] - 2.0 * (Xd @ Xd.T)
