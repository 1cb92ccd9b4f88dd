"""GPU: the one-pass resident-centre Lloyd step (`kmeans_step_resident`)
against int64 / f64 numpy, its legality gate, and a fit that runs on it."""

import numpy as np
import pytest
import torch

import spark_rapids_ml_amd.ops.kmeans as km
from spark_rapids_ml_amd.ops import torch_ref

pytestmark = pytest.mark.gpu

TILE = km._KR_ROWS


@pytest.fixture(scope="module")
def ext():
    from spark_rapids_ml_amd.ops.dispatch import hip_ops

    return hip_ops()


def _two_tiles():
    """Rows that give block 0 a second, partial tile: the grid is
    min(#tiles, #CUs), so one tile more than CUs, 5 rows of it used."""
    return TILE * torch.cuda.get_device_properties(0).multi_processor_count + 5


def _step(ext, X, C):
    Xd, Cd = torch.from_numpy(X).cuda(), torch.from_numpy(C).cuda()
    out = ext.kmeans_step_resident(Xd, Cd, (Xd * Xd).sum(dim=1))
    return [o.cpu().numpy() for o in out]


def _from_labels(X, labels, k):
    sums = np.zeros((k, X.shape[1]), dtype=np.float64)
    np.add.at(sums, labels, X.astype(np.float64))
    return sums, np.bincount(labels, minlength=k).astype(np.float64)


# (n, k, d, how C and X are drawn)
EXACT = [
    (1, 1, 1, "uniform"),
    (63, 31, 3, "uniform"),
    (65, 33, 30, "uniform"),
    (65, 1, 130, "uniform"),
    (63, 33, 130, "uniform"),
    (1, 200, 128, "uniform"),
    (65, 200, 128, "uniform"),
    (63, 31, 128, "uniform"),
    (65, 200, 1, "uniform"),
    (63, 200, 30, "uniform"),
    (-1, 200, 128, "uniform"),   # two tiles in one block, the last partial
    (-1, 33, 3, "uniform"),
    (65, 33, 30, "unpicked"),    # every third centre far from all rows
    (65, 33, 30, "origin"),      # rows near 0, real centres far: a zero pad centre would win
]


@pytest.mark.parametrize("n,k,d,kind", EXACT)
def test_exact_integer_step(ext, n, k, d, kind):
    n = _two_tiles() if n < 0 else n
    rng = np.random.default_rng(n + 1000 * k + d)
    X = rng.integers(-8, 9, size=(n, d))
    C = rng.integers(-8, 9, size=(k, d))
    if kind == "unpicked":
        X = rng.integers(-1, 2, size=(n, d))
        C[::3] = 8
    elif kind == "origin":
        X = rng.integers(-1, 2, size=(n, d))
        C = rng.choice([-8, 8], size=(k, d))
    labels, sums, counts, inertia = _step(ext, X.astype(np.float32), C.astype(np.float32))
    D = (X * X).sum(1)[:, None] + (C * C).sum(1)[None, :] - 2 * (X @ C.T)  # int64, exact
    assert labels.min() >= 0 and labels.max() < k
    own = D[np.arange(n), labels]
    assert np.array_equal(own, D.min(axis=1))
    ref_sums, ref_counts = _from_labels(X, labels, k)
    assert np.array_equal(sums, ref_sums)
    assert np.array_equal(counts, ref_counts)
    assert inertia[0] == float(own.sum())
    if kind == "unpicked":
        assert (counts[::3] == 0).all() and (sums[::3] == 0).all()


def _check_float(X, C, labels, sums, counts, inertia):
    """The assertions of the float step: every row within the f32 dot-product
    bound of its f64 minimum; sums, counts, inertia against f64 from the labels."""
    X64, C64 = X.astype(np.float64), C.astype(np.float64)
    k, d = C.shape
    D = (X64 * X64).sum(1)[:, None] + (C64 * C64).sum(1)[None, :] - 2.0 * (X64 @ C64.T)
    own = D[np.arange(len(X)), labels]
    u = 2.0 ** -24
    gamma = (d + 2) * u / (1.0 - (d + 2) * u)
    bound = 4.0 * gamma * np.linalg.norm(X64, axis=1) * np.linalg.norm(C64, axis=1).max()
    assert (own <= D.min(axis=1) + bound).all()
    ref_sums, ref_counts = _from_labels(X, labels, k)
    assert np.array_equal(counts, ref_counts)
    # relative to the largest entry: an entry that cancels to ~0 has no
    # relative accuracy of its own in any summation order
    assert np.abs(sums - ref_sums).max() <= 1e-5 * np.abs(ref_sums).max()
    assert abs(float(inertia) - own.sum()) <= 1e-5 * own.sum()


def _d_max(k):
    return max(d for d in range(1, 1025) if km._resident_lds_bytes(k, d))


@pytest.mark.parametrize("n,k,d", [(5000, 200, 128), (777, 40, -1)])
def test_float_step_against_f64(ext, n, k, d):
    d = _d_max(k) if d < 0 else d  # the widest rows whose tile still fits beside k centres
    rng = np.random.default_rng(7)
    X = rng.standard_normal((n, d)).astype(np.float32)
    C = rng.standard_normal((k, d)).astype(np.float32)
    labels, sums, counts, inertia = _step(ext, X, C)
    _check_float(X, C, labels, sums, counts, inertia[0])


def test_gate(ext, monkeypatch):
    d = 128
    k_max = max(k for k in range(1, 384) if km._resident_lds_bytes(k, d))
    for k in (1, 31, 200, k_max, k_max + 1, 383):
        for dd in (1, 3, 128, 129, 130, 316, 317, 425):
            assert ext.kmeans_resident_lds_bytes(k, dd) == km._resident_lds_bytes(k, dd)
    rng = np.random.default_rng(3)
    X = rng.standard_normal((1000, d)).astype(np.float32)
    C = rng.standard_normal((k_max + 1, d)).astype(np.float32)
    labels, sums, counts, inertia = _step(ext, X, C[:k_max])  # the largest legal k launches
    _check_float(X, C[:k_max], labels, sums, counts, inertia[0])
    with pytest.raises(RuntimeError, match="not legal"):
        _step(ext, X, C)
    # the first illegal shape falls back to the GEMM + argmin + accumulate path
    monkeypatch.setenv("SRML_KMEANS_VARIANT", "resident")
    Xd, Cd = torch.from_numpy(X).cuda(), torch.from_numpy(C).cuda()
    assert km._resident_wanted(Xd, Cd[:k_max]) and not km._resident_wanted(Xd, Cd)
    labels, sums, counts, inertia = km.kmeans_assign_reduce(Xd, Cd)
    _check_float(X, C, labels.cpu().numpy(), sums.cpu().numpy(), counts.cpu().numpy(), inertia)


def test_fit_runs_on_resident_kernel(monkeypatch):
    from spark_rapids_ml_amd import KMeans
    from spark_rapids_ml_amd.data import DataFrame

    rng = np.random.default_rng(0)
    centres = 20.0 * rng.standard_normal((5, 16))
    X = (centres[rng.integers(0, 5, size=2000)] + rng.standard_normal((2000, 16))).astype(np.float32)
    seen = []
    real = km._step_resident

    def counted(ext, Xt, C, x_sq):
        seen.append(C.detach().double().cpu())
        return real(ext, Xt, C, x_sq)

    import spark_rapids_ml_amd.models.clustering as clustering

    steps = []

    def step(*args):
        steps.append(1)
        return km.kmeans_assign_reduce(*args)

    monkeypatch.setenv("SRML_KMEANS_VARIANT", "resident")
    monkeypatch.setattr(km, "_step_resident", counted)
    monkeypatch.setattr(clustering, "kmeans_assign_reduce", step)
    model = KMeans(k=5, maxIter=10, seed=1).fit(DataFrame.from_numpy(X))
    n_iter = model.summary.numIter
    # the kernel served every step of the fit: the k-means|| candidate
    # weighting (one call) and then exactly the Lloyd steps
    assert n_iter >= 1 and len(steps) == len(seen) == n_iter + 1
    assert all(C.shape == (5, 16) for C in seen[1:])
    X64 = torch.from_numpy(X).double()
    C = seen[1]  # the centres the first Lloyd step started from
    for _ in range(n_iter):
        _l, sums, counts, _i = torch_ref.kmeans_assign_reduce(X64, C, (X64 * X64).sum(dim=1))
        C = torch.where(counts[:, None] > 0, sums / counts.clamp(min=1)[:, None], C)
    assert np.abs(model.cluster_centers_ - C.numpy()).max() <= 1e-4
