"""RandomForest entropy impurity and class counts past 16: the
rf_best_split_scan and fil_predict_wide kernels against plain float64
references, and the criterion from the estimator down to the saved model."""

import os

import numpy as np
import pytest
import torch

from spark_rapids_ml_amd import RandomForestClassifier, RandomForestRegressor
from spark_rapids_ml_amd.data import DataFrame
from spark_rapids_ml_amd.models.tree import _grow_forest
from spark_rapids_ml_amd.ops.forest import forest_traverse

# the project's kernel-vs-f64 gain bound (tests/test_forest_grow.py)
GAIN_RTOL, GAIN_ATOL = 1e-4, 1e-5

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def ext():
    from spark_rapids_ml_amd.ops.dispatch import hip_ops

    return hip_ops()


def _close(got, ref):
    return abs(got - ref) <= GAIN_ATOL + GAIN_RTOL * abs(ref)


def _phi_sum(counts, criterion):
    """sum_c phi(x_c) over the last axis: x^2 (gini) or x*log2(x), phi(0) = 0."""
    x = np.asarray(counts, np.float64)
    if criterion == "gini":
        return (x * x).sum(axis=-1)
    return (x * np.log2(np.where(x > 0, x, 1.0))).sum(axis=-1)


def _gains(left, total, criterion):
    """f64 gain of splitting class counts `total` [..., C] into `left` and
    total - left; nan where a side is empty."""
    right = total - left
    l, r, t = left.sum(-1), right.sum(-1), total.sum(-1)
    sL, sR, sT = (_phi_sum(v, criterion) for v in (left, right, total))
    with np.errstate(divide="ignore", invalid="ignore"):
        if criterion == "gini":
            # g_p - (l/t) g_l - (r/t) g_r with g_x = 1 - S_x / x^2
            g = (1 - sT / t**2) - l / t * (1 - sL / l**2) - r / t * (1 - sR / r**2)
        else:
            g = ((t * np.log2(t) - sT) - (l * np.log2(l) - sL) - (r * np.log2(r) - sR)) / t
    return np.where((l > 0) & (r > 0), g, np.nan)


# ---------------------------------------------------------------------------
# 1. split scan against an f64 cumsum
# ---------------------------------------------------------------------------


@gpu
@pytest.mark.parametrize("unsat", [False, True], ids=["leaf1", "leaf-unsat"])
@pytest.mark.parametrize("F", [1, 5])
@pytest.mark.parametrize("nb", [8, 65, 256])
@pytest.mark.parametrize("C", [2, 16, 17, 70])
@pytest.mark.parametrize("criterion", ["gini", "entropy"])
def test_split_scan_matches_f64(ext, criterion, C, nb, F, unsat):
    rng = np.random.default_rng(C * 1000 + nb + F)
    H = rng.integers(0, 6, size=(3, F, nb, C)).astype(np.float64)
    H[1] = 0.0  # an empty node
    min_leaf = int(H.sum(axis=(2, 3)).max()) if unsat else 1
    gain, feat, sbin, lval, rval = (
        t.cpu().numpy()
        for t in ext.rf_best_split_scan(
            torch.from_numpy(H).float().cuda(), min_leaf, ["gini", "entropy"].index(criterion)
        )
    )
    cs = H.cumsum(axis=2)
    total, left = cs[:, :, -1:, :], cs[:, :, :-1, :]
    ref = _gains(left, total, criterion)  # [3, F, nb-1]
    lc, rc = left.sum(-1), (total - left).sum(-1)
    ref = np.where((lc >= min_leaf) & (rc >= min_leaf) & ~np.isnan(ref), ref, -1.0)
    for b in range(3):
        best = ref[b].max()
        print(f"node {b}: gain {gain[b]!r} ref {best!r} at ({feat[b]}, {sbin[b]})")
        if best < 0:  # no valid boundary
            assert (gain[b], feat[b], sbin[b]) == (-1.0, -1, -1)
            assert not lval[b].any() and not rval[b].any()
            continue
        assert not unsat and b != 1
        assert _close(float(gain[b]), best)
        assert _close(ref[b, feat[b], sbin[b]], best)
        assert np.array_equal(lval[b], left[b, feat[b], sbin[b]])
        assert np.array_equal(rval[b], (total - left)[b, feat[b], sbin[b]])


# ---------------------------------------------------------------------------
# 2. grown trees under entropy
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("device", ["cpu", pytest.param("cuda", marks=gpu)])
@pytest.mark.parametrize("C", [3, 17])
def test_grown_trees_entropy_gain(C, device):
    n, d, nb, n_trees = 300, 4, 8, 2
    rng = np.random.default_rng(C)
    Xb = rng.integers(0, nb, size=(n, d), dtype=np.uint8)
    y = (Xb[:, 0].astype(np.int64) + 2 * Xb[:, 1] + rng.integers(0, 2, size=n)) % C
    gen = torch.Generator(device=device)
    gen.manual_seed(7)
    edges = torch.arange(1, nb, dtype=torch.float32).repeat(d, 1).to(device)
    trees = _grow_forest(
        torch.from_numpy(Xb).to(device), torch.from_numpy(y).to(device), edges,
        "classification", C, nb, 3, 1, 0.0, d, gen, n_trees=n_trees, criterion="entropy",
    )
    # brute-force best root gain over all (feature, bin): no bootstrap, so
    # every tree's root holds all rows
    H = np.zeros((d, nb, C))
    for f in range(d):
        np.add.at(H[f], (Xb[:, f], y), 1.0)
    cs = H.cumsum(axis=1)
    root_best = np.nanmax(_gains(cs[:, :-1], cs[:, -1:], "entropy"))
    n_internal = 0
    for tr in trees:
        val = tr["value"].astype(np.float64)
        assert _close(float(tr["gain"][0]), root_best), (tr["gain"][0], root_best)
        for node in np.nonzero(~tr["is_leaf"])[0]:
            ref = float(_gains(val[tr["left"][node]], val[node], "entropy"))
            assert np.array_equal(val[node], val[tr["left"][node]] + val[tr["right"][node]])
            assert _close(float(tr["gain"][node]), ref), (node, tr["gain"][node], ref)
            n_internal += 1
    assert n_internal > 0


# ---------------------------------------------------------------------------
# 3. estimator surface
# ---------------------------------------------------------------------------


def test_estimator_impurity(tmp_path):
    import pyarrow.parquet as pq

    rng = np.random.default_rng(0)
    X = rng.normal(size=(200, 4)).astype(np.float32)
    y = ((X[:, 0] > 0).astype(np.int64) + (X[:, 1] > 0.5)).astype(np.float64)
    df = DataFrame.from_numpy(X, y)
    kw = dict(numTrees=2, maxDepth=3, seed=1)
    model = RandomForestClassifier(impurity="entropy", **kw).fit(df)
    assert model.getOrDefault("impurity") == "entropy"
    with pytest.raises(ValueError, match="variance"):
        RandomForestRegressor(impurity="entropy", **kw).fit(df)
    with pytest.raises(ValueError, match="gini.*entropy"):
        RandomForestClassifier(impurity="variance", **kw).fit(df)

    p = str(tmp_path / "rfc")
    model.saveAsSparkModel(p)
    with open(os.path.join(p, "metadata", "part-00000")) as f:
        assert '"impurity":"entropy"' in f.readline().replace(" ", "")
    rows = pq.read_table(os.path.join(p, "data")).to_pylist()
    assert any(r["nodeData"]["impurity"] > 0 for r in rows)
    for r in rows:
        v = np.asarray(r["nodeData"]["impurityStats"], np.float64)
        pr = v[v > 0] / v.sum()
        assert abs(r["nodeData"]["impurity"] + (pr * np.log2(pr)).sum()) <= 1e-12


# ---------------------------------------------------------------------------
# 4. wide inference, exact
# ---------------------------------------------------------------------------


def _wide_forest(rng, T, C, d):
    """T complete trees of depth 0..3 (tree 0 is a bare root leaf). Leaf
    counts sum to 8 or 16: every vote is dyadic, the f32 sum over trees exact."""
    trees = []
    for t in range(T):
        depth = 0 if t == 0 else 1 + t % 3
        m = 2 ** (depth + 1) - 1
        leaf = np.arange(m) >= m // 2
        kids = np.where(leaf, -1, 2 * np.arange(m) + 1)
        value = np.zeros((m, C), np.float32)
        for i in np.nonzero(leaf)[0]:
            value[i] = rng.multinomial(int(rng.choice([8, 16])), np.full(C, 1.0 / C))
        trees.append({
            "feature": np.where(leaf, -1, rng.integers(0, d, m)).astype(np.int32),
            "threshold": rng.integers(1, 8, m).astype(np.float32),
            "left": kids.astype(np.int32),
            "right": np.where(leaf, -1, kids + 1).astype(np.int32),
            "is_leaf": leaf,
            "value": value,
        })
    return trees


@gpu
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("T", [1, 64, 65])
@pytest.mark.parametrize("C", [17, 64, 65, 130])
def test_fil_predict_wide_exact(ext, C, T, n):
    d = 3
    rng = np.random.default_rng(C + T)
    trees = _wide_forest(rng, T, C, d)
    X = rng.integers(0, 8, size=(n, d)).astype(np.float32)  # x == thr goes right
    ref = np.zeros((n, C), np.float64)
    for i in range(n):
        for t in trees:
            node = 0
            while not t["is_leaf"][node]:
                go_left = X[i, t["feature"][node]] < t["threshold"][node]
                node = t["left"][node] if go_left else t["right"][node]
            ref[i] += t["value"][node].astype(np.float64) / t["value"][node].sum()
    cat = lambda key: torch.from_numpy(np.concatenate([t[key] for t in trees])).cuda()  # noqa: E731
    sizes = [len(t["feature"]) for t in trees]
    roots = torch.from_numpy(np.cumsum([0] + sizes[:-1]).astype(np.int64)).cuda()
    out = ext.fil_predict_wide(
        torch.from_numpy(X).cuda(), cat("feature"), cat("threshold"), cat("left"),
        cat("right"), cat("value"), roots,
    ).cpu()
    assert np.array_equal(out.numpy().astype(np.float64), ref)
    if (C, T, n) == (65, 65, 5):
        assert torch.equal(out, forest_traverse(torch.from_numpy(X), trees, "classification", C))
