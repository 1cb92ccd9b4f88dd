"""`moments_f64` ([X | 1 | y]ᵀ[X | 1 | y] on f64 MFMA) against int64 and
longdouble numpy, the fits that reach it, and the torch expressions it leaves
to every other dtype and device."""

import numpy as np
import pytest
import torch

from spark_rapids_ml_amd.ops import linalg, torch_ref

gpu = pytest.mark.gpu
U = 2.0 ** -53


@pytest.fixture(scope="module")
def ext():
    from spark_rapids_ml_amd.ops.dispatch import hip_ops

    return hip_ops()


def _data(n, d, with_y, kind):
    """Z = [X | 1 | y]: integers in [-8, 8], or floats 1e4 + N(0, 1)."""
    rng = np.random.default_rng(1000 * n + 2 * d + with_y)
    if kind == "int":
        X, y = rng.integers(-8, 9, (n, d)), rng.integers(-8, 9, n)
    else:
        X, y = 1e4 + rng.standard_normal((n, d)), 1e4 + rng.standard_normal(n)
    cols = [X, np.ones((n, 1), X.dtype)] + ([y[:, None]] if with_y else [])
    return X, (y if with_y else None), np.concatenate(cols, axis=1)


def _run(ext, X, y):
    Xd = torch.from_numpy(X).double().cuda()
    return ext.moments_f64(Xd, None if y is None else torch.from_numpy(y).double().cuda())


# (n, d, with_y): one below, at and above each edge of the 128-wide tiles
EXACT = [
    (1, 1, False),      # da = 2: a lone diagonal tile, one ragged panel
    (15, 3, True),      # da = 5, scalar loads
    (16, 128, False),   # da = 129: the off-diagonal tile holds only the ones column
    (17, 127, True),    # da = 129: y alone in the second stripe, scalar loads
    (33, 126, True),    # da = 128: ones and y end the lone tile, double2 pairs (1, y)
    (33, 129, True),    # odd d, scalar loads, X reaches into the second stripe
    (31, 131, False),   # odd d, scalar loads, no y
    (300, 257, True),   # three stripes, six tiles, several panels, scalar loads
    (300, 256, True),   # the same on double2 loads; (1, y) open the third stripe
    (5003, 5, True),    # split 53 (3 panels a slice), last slice one panel of 11 rows
    (5003, 130, False), # split above 1 over three tiles, double2 loads, (1, 0) pair
    (0, 4, False),      # no launch, zeros
]


@gpu
@pytest.mark.parametrize("n,d,with_y", EXACT)
def test_exact_integer_moments(ext, n, d, with_y):
    X, y, Z = _data(n, d, with_y, "int")
    M = _run(ext, X, y).cpu().numpy()
    # integers below 2^53 whatever the order: exact, and so exactly symmetric
    assert np.array_equal(M, Z.astype(np.int64).T @ Z.astype(np.int64))


@gpu
def test_float_moments_within_the_dot_product_bound(ext):
    n = 1000
    X, y, Z = _data(n, 130, True, "float")
    M = _run(ext, X, y).cpu().numpy()
    Zl = Z.astype(np.longdouble)
    gamma = n * U / (1 - n * U)
    ratio = np.abs(M - Zl.T @ Zl) / (gamma * (np.abs(Zl).T @ np.abs(Zl)))
    print("worst error / bound", float(ratio.max()))
    assert ratio.max() <= 1.0


@gpu
def test_repeatable_with_a_row_split(ext):
    X, y, _ = _data(5003, 5, True, "float")
    assert torch.equal(_run(ext, X, y), _run(ext, X, y))


@gpu
def test_f64_fits_run_on_the_kernel(ext, monkeypatch):
    """Both f64 fits complete without torch's Gram and agree with centred
    numpy f64 within c·n·u·μ²/gap. The intercept ȳ − x̄ᵀw carries the
    coefficient error times ‖x̄‖₁ = 2e4, so it is the sharp one: it holds only
    while the Gram is good to about an ulp (64-row slices, compensated
    reduce; 288-row slices added plainly miss it five times over)."""
    from spark_rapids_ml_amd import PCA, LinearRegression
    from spark_rapids_ml_amd.data import DataFrame

    def no_gram(X):
        raise AssertionError("the f64 fit formed its Gram in torch")

    monkeypatch.setattr(torch_ref, "gram", no_gram)
    n, d, mu = 2000, 20, 1e3
    rng = np.random.default_rng(7)
    X = mu + rng.standard_normal((n, d)) * np.sqrt(0.8 ** np.arange(d))
    y = (X - mu) @ rng.standard_normal(d) + 0.1 * rng.standard_normal(n)
    Xc = X - X.mean(0)
    lam, V = np.linalg.eigh(Xc.T @ Xc / (n - 1))  # ascending
    c = 10.0

    pca = PCA(k=2, float32_inputs=False).fit(DataFrame.from_numpy(X))
    tol = c * n * U * mu ** 2 / min(lam[-1] - lam[-2], lam[-2] - lam[-3])
    for got, want in zip(pca.components_, V[:, ::-1].T):
        err = min(np.abs(got - want).max(), np.abs(got + want).max())
        print("pca component err", err, "tol", tol)
        assert err <= tol

    lr = LinearRegression(float32_inputs=False).fit(DataFrame.from_numpy(X, y))
    w = np.linalg.lstsq(Xc, y - y.mean(), rcond=None)[0]
    b = y.mean() - X.mean(0) @ w
    tol = c * n * U * mu ** 2 / lam[0]
    print("coef err", np.abs(lr.coefficients - w).max(), "intercept err", abs(lr.intercept - b), "tol", tol)
    assert np.abs(lr.coefficients - w).max() <= tol
    assert abs(lr.intercept - b) <= tol


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("with_y", [False, True])
@pytest.mark.parametrize("switch", [None, "0"])
def test_cpu_moments_are_the_inline_expressions(monkeypatch, dtype, with_y, switch):
    if switch is not None:
        monkeypatch.setenv("SRML_MOMENTS_F64", switch)
    X, y, _ = _data(300, 19, with_y, "float")
    Xt = torch.from_numpy(X).to(dtype)
    yt = torch.from_numpy(y).to(dtype) if with_y else None
    G, xsum, Xty, ysum, y2sum = linalg.moments(Xt, yt)
    assert torch.equal(G, linalg.gram(Xt).to(torch.float64))
    assert torch.equal(xsum, Xt.sum(dim=0).to(torch.float64))
    if not with_y:
        assert Xty is None and ysum is None and y2sum is None
        return
    assert torch.equal(Xty, (Xt.T @ yt).to(torch.float64))
    assert torch.equal(ysum, yt.sum().to(torch.float64))
    assert torch.equal(y2sum, (yt * yt).sum().to(torch.float64))
