"""Grown trees are correct: every tree `_grow_forest` returns is replayed in
numpy from the root and each node is checked against the rows that reach it.

Inputs are built so that everything is exact: `Xb` holds the bins themselves
and `edges = arange(1, nb)`, so a stored threshold t means `bin <= t - 1` and
a tree can be replayed on `Xb`. Regression targets are integers in [-8, 8]
with max|y| = 8 and n <= 512: the histogram kernel's Q14 fixed-point cells
(quantum 8/16384 = 2^-11) and its cross-block float atomics then add exactly
(n * 8 * 2^11 < 2^24), so the GPU sums are deterministic and true.
"""

import numpy as np
import pytest
import torch

from spark_rapids_ml_amd.models.tree import _grow_forest

# kernel-vs-torch gain tolerance of test_rf_best_split_matches_ref; the
# brute-force reference below is float64, the code under test float32.
# Measured before the grower was split: the largest deviation over all cases
# is 2.4 % of this bound on both the CPU and the MI355X (reg-multibatch).
GAIN_RTOL, GAIN_ATOL = 1e-4, 1e-5

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]

# task, C, n, d, nb, depth, min_leaf, trees, bootstrap, max_features, node_batch
CASES = {
    "clf-base": ("classification", 3, 400, 5, 8, 4, 2, 3, False, 5, 16384),
    "clf-multibatch": ("classification", 3, 400, 5, 8, 4, 2, 3, True, 5, 2),
    "clf-c17-torch-scan": ("classification", 17, 400, 5, 8, 4, 1, 2, True, 5, 16384),
    "clf-sampled": ("classification", 3, 400, 9, 8, 4, 2, 3, True, 3, 16384),
    "reg-base": ("regression", 0, 400, 5, 8, 4, 2, 3, False, 5, 16384),
    "reg-multibatch": ("regression", 0, 400, 5, 8, 4, 2, 3, True, 5, 2),
    "reg-sampled": ("regression", 0, 400, 9, 8, 4, 2, 3, True, 3, 16384),
}


def _inputs(task, C, n, d, nb, trees, bootstrap):
    rng = np.random.default_rng(1234)
    Xb = rng.integers(0, nb, size=(n, d), dtype=np.uint8)
    a, b = Xb[:, 0].astype(np.int64), Xb[:, 1].astype(np.int64)
    if task == "classification":
        y = (a + 2 * b + rng.integers(0, 2, size=n)) % C
    else:
        y = np.clip(a - b + rng.integers(-1, 2, size=n), -8, 8)
        y[0] = 8  # max|y| = 8 exactly: the Q14 quantum is then 2^-11
        y = y.astype(np.float32)
    sample = None
    if bootstrap:
        # per-tree sorted draws, as the estimator passes them
        sample = np.sort(rng.integers(0, n, size=(trees, n)), axis=1).astype(np.int32).ravel()
    return Xb, y, sample


def _best_gain_bruteforce(task, C, bins, y, nb, min_leaf):
    """Best gain over ALL (feature, bin) pairs that respect min_leaf, float64.
    bins: [m, d] rows at the node; criterion as in the split scan: Gini, or
    (ls^2/lc + rs^2/rc - ts^2/tc)/tc."""
    m, d = bins.shape
    best = -1.0
    for f in range(d):
        if task == "classification":
            H = np.zeros((nb, C), np.float64)
            np.add.at(H, (bins[:, f], y), 1.0)
        else:
            H = np.zeros((nb, 2), np.float64)
            np.add.at(H, (bins[:, f], 0), 1.0)
            np.add.at(H, (bins[:, f], 1), y.astype(np.float64))
        cs = H.cumsum(axis=0)
        tot = cs[-1]
        for b in range(nb - 1):
            left, right = cs[b], tot - cs[b]
            if task == "classification":
                lc, rc, tc = left.sum(), right.sum(), tot.sum()
            else:
                lc, rc, tc = left[0], right[0], tot[0]
            if lc < min_leaf or rc < min_leaf:
                continue
            if task == "classification":
                gini = lambda c, s: 1.0 - ((c / s) ** 2).sum()
                g = gini(tot, tc) - lc / tc * gini(left, lc) - rc / tc * gini(right, rc)
            else:
                g = (left[1] ** 2 / lc + right[1] ** 2 / rc - tot[1] ** 2 / tc) / tc
            best = max(best, g)
    return best


def _check_forest(case, device):
    task, C, n, d, nb, depth, min_leaf, n_trees, bootstrap, mf, node_batch = case
    Xb, y, sample = _inputs(task, C, n, d, nb, n_trees, bootstrap)
    gen = torch.Generator(device=device)
    gen.manual_seed(7)
    edges = torch.arange(1, nb, dtype=torch.float32).repeat(d, 1).to(device)
    trees = _grow_forest(
        torch.from_numpy(Xb).to(device),
        torch.from_numpy(y).to(device),
        edges,
        task,
        C,
        nb,
        depth,
        min_leaf,
        0.0,
        mf,
        gen,
        n_trees=n_trees,
        sample=None if sample is None else torch.from_numpy(sample).to(device),
        node_batch=node_batch,
    )
    assert len(trees) == n_trees

    n_internal = 0
    worst = 0.0  # largest |gain - brute| / (atol + rtol * |brute|)
    for t, tr in enumerate(trees):
        rows0 = np.arange(n) if sample is None else sample[t * n : (t + 1) * n].astype(np.int64)
        stack = [(0, rows0)]
        seen = 0
        while stack:
            node, rows = stack.pop()
            seen += 1
            yr = y[rows]
            val = tr["value"][node]
            if task == "classification":
                assert np.array_equal(val, np.bincount(yr, minlength=C).astype(np.float32)), (t, node)
            else:
                assert val[1] == len(rows), (t, node)
                mean = float(yr.astype(np.float64).mean())
                assert abs(float(val[0]) - mean) <= 1e-5 * abs(mean), (t, node, val[0], mean)
            if tr["is_leaf"][node]:
                continue
            n_internal += 1
            f, thr = int(tr["feature"][node]), float(tr["threshold"][node])
            assert 0 <= f < d and thr == int(thr), (t, node, f, thr)
            go_left = Xb[rows, f] <= int(thr) - 1
            lrows, rrows = rows[go_left], rows[~go_left]
            assert len(lrows) >= min_leaf and len(rrows) >= min_leaf, (t, node)
            if mf == d:
                ref = _best_gain_bruteforce(task, C, Xb[rows], yr, nb, min_leaf)
                got = float(tr["gain"][node])
                err = abs(got - ref)
                worst = max(worst, err / (GAIN_ATOL + GAIN_RTOL * abs(ref)))
                assert err <= GAIN_ATOL + GAIN_RTOL * abs(ref), (t, node, got, ref)
            stack.append((int(tr["left"][node]), lrows))
            stack.append((int(tr["right"][node]), rrows))
        assert seen == len(tr["feature"]), (t, seen)  # every node is reachable
    assert n_internal > 0
    print(f"internal={n_internal} worst gain deviation / tolerance = {worst:.3g}")


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("case", list(CASES), ids=list(CASES))
def test_grown_trees_replay(case, device):
    _check_forest(CASES[case], device)


@pytest.mark.gpu
@pytest.mark.parametrize("hist", ["old", "fw"])
@pytest.mark.parametrize("case", ["clf-sampled", "reg-sampled"])
def test_grown_trees_replay_hist_override(case, hist, monkeypatch):
    """Both histogram kernels see sorted and unsorted sampled subsets."""
    monkeypatch.setenv("SRML_RF_HIST", hist)
    _check_forest(CASES[case], "cuda")
