"""The f64 Lloyd step (`kmeans_assign_f64` + `label_accumulate_f64`) against
int64 / f64 numpy, the dispatch that leads to it, and the CPU path it agrees with."""

import numpy as np
import pytest
import torch

import spark_rapids_ml_amd.ops.kmeans as km
from spark_rapids_ml_amd.ops import torch_ref

gpu = pytest.mark.gpu
U = 2.0 ** -53


@pytest.fixture(scope="module")
def ext():
    from spark_rapids_ml_amd.ops.dispatch import hip_ops

    return hip_ops()


def _data(n, k, d, kind):
    """Integers in [-8, 8] for the exact kinds; `float`: tight blobs near 1,
    where an f32 |c|² decides most rows wrongly."""
    if kind == "float":
        rng = np.random.default_rng(n + k + d)
        cent = 20 * rng.standard_normal((k, d))
        lab = rng.integers(0, k, n)
        X = 1 + 1e-5 * (cent[lab] + rng.standard_normal((n, d)))
        return X, 1 + 1e-5 * (cent + 0.1 * rng.standard_normal((k, d)))
    rng = np.random.default_rng(n + 1000 * k + d)
    X = rng.integers(-8, 9, size=(n, d))
    C = rng.integers(-8, 9, size=(k, d))
    if kind == "unpicked":  # every third centre far from all rows
        X = rng.integers(-1, 2, size=(n, d))
        C[::3] = 8
    elif kind == "origin":  # rows near 0, real centres far: a zero pad centre would win
        X = rng.integers(-1, 2, size=(n, d))
        C = rng.choice([-8, 8], size=(k, d))
    elif kind == "ties":  # every row has an exact tie; the lower index must win
        C[1::2] = C[0::2][: k // 2]
    return X, C


def _check(X, C, labels, sums, counts, inertia, min_dists=None):
    """Labels are the first-index argmin of the direct-difference distances;
    inertia, sums and counts within the f64 rounding model (exact for integers)."""
    (n, d), k = X.shape, C.shape[0]
    D = ((X[:, None] - C[None]) ** 2).sum(2)
    assert np.array_equal(labels, D.argmin(axis=1))
    exact = X.dtype.kind == "i"
    gamma = 0.0 if exact else (d + 2) * U / (1 - (d + 2) * U)
    bound = 4 * gamma * np.linalg.norm(X, axis=1) * np.linalg.norm(C, axis=1).max()
    print("inertia err", abs(inertia - D.min(1).sum()), "bound", bound.sum())
    assert abs(inertia - D.min(1).sum()) <= bound.sum()
    if min_dists is not None:
        assert (np.abs(min_dists - D.min(1)) <= bound).all()
    ref, mag = np.zeros((k, d)), np.zeros((k, d))
    np.add.at(ref, labels, X)
    np.add.at(mag, labels, np.abs(X))
    m = np.bincount(labels, minlength=k).astype(np.float64)
    assert np.array_equal(counts, m)
    assert (np.abs(sums - ref) <= (0 if exact else 2 * U) * m[:, None] * mag).all()


def _step(ext, X, C):
    Xd, Cd = torch.from_numpy(X).double().cuda(), torch.from_numpy(C).double().cuda()
    labels, min_d, inertia = ext.kmeans_assign_f64(Xd, Cd, (Xd * Xd).sum(dim=1))
    sums, counts = ext.label_accumulate_f64(Xd, labels, C.shape[0])
    return [t.cpu().numpy() for t in (labels, sums, counts, inertia, min_d)]


# (n, k, d, kind): one below, at and above the 128 x 128 x 16 tile edges, and the
# accumulation kernel's paths (double2 or scalar loads, row groups, column passes)
EXACT = [
    (1, 1, 1, "uniform"),
    (127, 127, 3, "uniform"),
    (129, 129, 4, "uniform"),
    (129, 1, 5, "uniform"),
    (1, 257, 15, "uniform"),
    (127, 257, 17, "uniform"),
    (128, 128, 16, "uniform"),
    (129, 129, 1, "uniform"),
    (300, 5, 130, "uniform"),   # double2 loads, two row groups, 4 rows in flight
    (300, 5, 131, "uniform"),   # scalar loads, one row group
    (9, 3, 514, "uniform"),     # double2 loads, one row group
    (5, 2, 2049, "uniform"),    # scalar loads, a second column pass
    (5, 3, 4098, "uniform"),    # double2 loads, a second column pass
    (129, 129, 17, "unpicked"),
    (129, 127, 17, "origin"),
    (65, 129, 5, "origin"),
    (129, 130, 17, "ties"),
    (300, 37, 19, "ties"),
]


@gpu
@pytest.mark.parametrize("n,k,d,kind", EXACT)
def test_exact_integer_step(ext, n, k, d, kind):
    X, C = _data(n, k, d, kind)
    labels, sums, counts, inertia, min_d = _step(ext, X, C)
    _check(X, C, labels, sums, counts, inertia[0], min_d)
    if kind == "unpicked":
        assert (counts[::3] == 0).all() and (sums[::3] == 0).all()


FLOAT = [(300, 37, 19), (257, 130, 70)]


@gpu
@pytest.mark.parametrize("n,k,d", FLOAT)
def test_float_step_against_f64(ext, n, k, d):
    X, C = _data(n, k, d, "float")
    labels, sums, counts, inertia, min_d = _step(ext, X, C)
    _check(X, C, labels, sums, counts, inertia[0], min_d)
    again = _step(ext, X, C)  # no floating atomics: the same bits
    assert np.array_equal(labels, again[0]) and np.array_equal(sums, again[1])
    assert inertia[0] == again[3][0]


@gpu
def test_public_ops_take_the_f64_kernels(ext):
    X, C = _data(*FLOAT[0], "float")
    Xd, Cd = torch.from_numpy(X).cuda(), torch.from_numpy(C).cuda()
    labels, sums, counts, inertia = km.kmeans_assign_reduce(Xd, Cd)
    _check(X, C, labels.cpu().numpy(), sums.cpu().numpy(), counts.cpu().numpy(), inertia)
    want = ((X[:, None] - C[None]) ** 2).sum(2).argmin(1)
    assert np.array_equal(km.kmeans_predict(Xd, Cd).cpu().numpy(), want)


@gpu
def test_f64_fit_runs_on_the_kernel(ext, monkeypatch):
    from spark_rapids_ml_amd import KMeans
    from spark_rapids_ml_amd.data import DataFrame
    import spark_rapids_ml_amd.models.clustering as clustering

    rng = np.random.default_rng(0)
    centres = 20.0 * rng.standard_normal((5, 16))
    X = 1 + 1e-5 * (centres[rng.integers(0, 5, size=2000)] + rng.standard_normal((2000, 16)))
    seen, steps = [], []
    real = ext.kmeans_assign_f64

    def counted(Xt, C, x_sq):
        seen.append(C.detach().cpu().numpy())
        return real(Xt, C, x_sq)

    def step(*args):
        steps.append(1)
        return km.kmeans_assign_reduce(*args)

    monkeypatch.setattr(ext, "kmeans_assign_f64", counted)
    monkeypatch.setattr(clustering, "kmeans_assign_reduce", step)
    model = KMeans(k=5, maxIter=10, seed=1, float32_inputs=False).fit(DataFrame.from_numpy(X))
    n_iter = model.summary.numIter
    # the kernel served the k-means|| candidate weighting and every Lloyd step
    assert n_iter >= 1 and len(steps) == len(seen) == n_iter + 1
    C = seen[1]  # the centres the first Lloyd step started from
    for _ in range(n_iter):
        lab = ((X[:, None] - C[None]) ** 2).sum(2).argmin(1)
        C = np.stack([X[lab == j].mean(0) if (lab == j).any() else C[j] for j in range(5)])
    assert np.abs(model.cluster_centers_ - C).max() <= 1e-12
    sizes = model.summary.clusterSizes
    assert len(sizes) == 5 and min(sizes) > 0 and sum(sizes) == 2000


def test_cpu_path_is_f64_and_f32_unchanged():
    X, C = _data(*FLOAT[0], "float")
    Xt, Ct = torch.from_numpy(X), torch.from_numpy(C)
    labels, sums, counts, inertia = km.kmeans_assign_reduce(Xt, Ct)
    _check(X, C, labels.numpy(), sums.numpy(), counts.numpy(), inertia)
    # f32 rows keep the expansion they had: |x|² and |c|² formed in f32
    Xf, Cf = Xt.float(), Ct.float()
    got = torch_ref.kmeans_assign_reduce(Xf, Cf)
    old = torch_ref.kmeans_assign_reduce(Xf, Cf, (Xf.to(torch.float32) ** 2).sum(dim=1))
    assert torch.equal(got[0], old[0]) and torch.equal(got[1], old[1]) and got[3] == old[3]
