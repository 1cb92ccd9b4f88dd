"""`logreg_grad_loss_f64` (logistic loss and gradient on f64 MFMA) against
longdouble numpy and exact integers, the fit that reaches it, and the
expressions `logistic_grad_loss` leaves to every other dtype and device."""

import numpy as np
import pytest
import torch

from spark_rapids_ml_amd.ops import glm, torch_ref

gpu = pytest.mark.gpu
U = 2.0 ** -53
LD = np.longdouble
C_E = 1.0  # roundings of exp, log and the divide, in ulps; see test_within_the_forward_error_bound


@pytest.fixture(scope="module")
def ext():
    from spark_rapids_ml_amd.ops.dispatch import hip_ops

    return hip_ops()


def _data(n, d, C, icpt, scale=1.0, ints=False):
    rng = np.random.default_rng(100000 * C + 100 * n + 2 * d + icpt)
    X = rng.integers(-8, 9, (n, d)).astype(np.float64) if ints else rng.standard_normal((n, d))
    W = np.zeros((C, d + icpt)) if ints else scale * rng.standard_normal((C, d + icpt)) / np.sqrt(d)
    return X, rng.integers(0, max(C, 2), n), W


def _ref(X, y, W, icpt, c_e):
    """Longdouble (grad, loss) and their forward-error bounds (below)."""
    n, d = X.shape
    C = W.shape[0]
    gam = lambda m: m * U / (1 - m * U)
    Xa = np.concatenate([X, np.ones((n, 1))], axis=1).astype(LD) if icpt else X.astype(LD)
    S, eS = Xa @ W.T.astype(LD), gam(d + 2) * (np.abs(Xa) @ np.abs(W.T).astype(LD))
    if C == 1:  # the sigmoid is the softmax over (z, 0), label 1 being class 0 there
        S, eS = np.concatenate([S, 0 * S], axis=1), np.concatenate([eS, 0 * eS], axis=1)
        y = 1 - y
    Cs = S.shape[1]
    mx = S.max(axis=1, keepdims=True)
    E = np.exp(S - mx)
    den = E.sum(axis=1, keepdims=True)
    P = E / den
    rel = 2 * eS.max(axis=1, keepdims=True) + U * (np.abs(S - mx) + Cs + c_e)
    sy = np.take_along_axis(S, y[:, None], axis=1)
    li = (np.log(den) - (sy - mx))[:, 0]
    eli = (P * rel).sum(axis=1) + eS.max(axis=1) + U * (np.abs(np.log(den)) + np.abs(sy - mx))[:, 0]
    R = P - (np.arange(Cs)[None, :] == y[:, None])
    eR = P * rel + U * np.abs(R)
    if C == 1:
        R, eR = R[:, :1], eR[:, :1]
    G = R.T @ Xa
    eG = eR.T @ np.abs(Xa) + gam(n) * (np.abs(R).T @ np.abs(Xa))
    return G, li.sum(), eG, eli.sum() + gam(n) * np.abs(li).sum()


def _run(fn, X, y, W, icpt):
    g, l = fn(torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda(), torch.from_numpy(W).cuda(), icpt)
    return g.cpu().numpy(), float(l)


def _ratios(got, X, y, W, icpt, c_e):
    G, L, eG, eL = _ref(X, y, W, icpt, c_e)
    return float((np.abs(got[0] - G) / eG).max()), float(abs(got[1] - L) / eL)


# (n, d, C, fit_intercept, W scale): one below, at and above the 128-row
# block, the 32-column panel, the 64-column stripe and its 32-column pair-tiles
BOUND = [
    (1, 1, 1, True, 1),        # one row, ka = 2, sigmoid
    (15, 3, 2, False, 1),      # odd d: scalar loads
    (17, 127, 3, True, 1),     # ka = 128: the intercept ends the second stripe
    (300, 128, 16, True, 1),   # double2 loads; the intercept alone opens a panel and a stripe
    (300, 129, 17, False, 1),  # two class tiles, one class in the second
    (300, 256, 33, True, 1),   # four class tiles, ka = 257
    (300, 257, 64, False, 1),  # every class live, scalar loads, five stripes
    (5003, 128, 3, True, 1),   # 53 row slices, the last one short
    (5003, 31, 1, True, 1),    # ka = 32: the intercept ends the lone panel; sigmoid
    (129, 32, 10, True, 1),    # one row into the second block; ka = 33
    (127, 64, 64, True, 1),    # ka = 65 with 16-row batches
    (300, 64, 10, True, 50),   # scores reach +-100: only a stable softmax survives
]


@gpu
@pytest.mark.parametrize("n,d,C,icpt,scale", BOUND)
def test_within_the_forward_error_bound(ext, n, d, C, icpt, scale):
    """With u = 2^-53 and γ_m = m·u / (1 − m·u): a score carries at most
    e_s = γ_{d+2} Σ_j |x_ij||w_cj| (a d(+1)-term dot product in any order). A
    probability exp(s_c − m) / Σ exp(s_c' − m) then has the relative error
    2·max_c e_s (numerator and denominator each move by a score error) plus
    u·(|s_c − m| + C + c_e): the argument's rounding scaled by the exponent,
    the C-term sum, and c_e for the roundings of exp, log and the divide.
    Residual: that times p, plus u·|r| for the subtraction. Gradient: the
    residual errors through |X|, plus γ_n |R|ᵀ|X| for the n-term sums. Loss of
    a row, log Σ − (s_y − m): the p-weighted relative error of Σ, one score
    error, u·(|log Σ| + |s_y − m|); summed, plus γ_n Σ|l_i|. The sigmoid is
    the softmax over (z, 0). Measured on MI355X with c_e = 0: worst ratio
    0.073 (gradient) and 0.068 (loss), RESULTS.md; that already leaves a
    factor 4, so C_E = 1, the smallest power of two that is a whole ulp."""
    X, y, W = _data(n, d, C, icpt, scale)
    got = _run(ext.logreg_grad_loss_f64, X, y, W, icpt)
    print("worst error / bound with c_e = 0 (grad, loss)", _ratios(got, X, y, W, icpt, 0.0))
    rg, rl = _ratios(got, X, y, W, icpt, C_E)
    print("worst error / bound (grad, loss)", rg, rl)
    assert rg <= 1.0 and rl <= 1.0


# (n, d, C, fit_intercept)
EXACT = [(17, 3, 1, True), (5003, 31, 1, True), (300, 129, 2, False), (5003, 128, 4, True),
         (300, 257, 16, True), (129, 64, 64, True), (0, 5, 4, True)]


@gpu
@pytest.mark.parametrize("n,d,C,icpt", EXACT)
def test_exact_at_zero_weights(ext, n, d, C, icpt):
    """W = 0: every probability is 1/C (1/2 for the sigmoid), a power of two,
    so R and G are exact whatever the summation order."""
    X, y, W = _data(n, d, C, icpt, ints=True)
    G, loss = _run(ext.logreg_grad_loss_f64, X, y, W, icpt)
    Xa = np.concatenate([X, np.ones((n, 1))], axis=1).astype(np.int64) if icpt else X.astype(np.int64)
    Cs = max(C, 2)
    hot = (np.arange(Cs)[None, :] == (1 - y if C == 1 else y)[:, None]).astype(np.int64)
    want = ((1 - Cs * hot).T @ Xa) / Cs  # (1/C − onehot)ᵀ [X | 1]; the sigmoid's row is label 1
    assert np.array_equal(G, want[:1] if C == 1 else want)
    assert abs(loss - n * np.log(Cs)) <= n * U / (1 - n * U) * n * np.log(Cs)


@gpu
def test_repeatable_with_a_row_split(ext):
    X, y, W = _data(5003, 128, 3, True)
    a, b = (ext.logreg_grad_loss_f64(torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda(),
                                     torch.from_numpy(W).cuda(), True) for _ in range(2))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@gpu
@pytest.mark.parametrize("classes", [3, 2])
def test_f64_fit_runs_on_the_kernel_to_the_f64_optimum(ext, monkeypatch, classes):
    """The fit completes without either softmax-residual path and stops where
    the gradient of the full objective, evaluated in longdouble at the
    returned coefficients, is at the f64 noise floor. The reference is the
    same fit on the CPU backend (f64 torch throughout) before this kernel
    existed: gradient norm 1.68e-11 (three classes, 32 iterations) and
    6.77e-15 (binary, 19 iterations) where its line search can no longer see
    the objective fall. The GPU fit is allowed 100 times that, as L-BFGS's
    stopping point at the floor depends on the summation order. What the f32
    residual it replaces reached is in RESULTS.md."""
    from spark_rapids_ml_amd import LogisticRegression
    from spark_rapids_ml_amd.data import DataFrame

    def no(*a, **k):
        raise AssertionError("the f64 fit left the f64 kernel")

    monkeypatch.setattr(ext, "softmax_residual_loss", no)
    monkeypatch.setattr(torch_ref, "softmax_residual", no)
    X, y, lam = *_fit_data(classes), 0.01
    m = LogisticRegression(float32_inputs=False, regParam=lam, tol=0, maxIter=500).fit(
        DataFrame.from_numpy(X, y.astype(np.float64)))
    norm = _objective_grad_norm(X, y, m.coefficientMatrix, m.interceptVector, lam)
    print("gradient norm at the fit", norm)
    assert norm <= 100 * {3: 1.68e-11, 2: 6.77e-15}[classes]


def _fit_data(classes, n=2000, d=10):
    rng = np.random.default_rng(classes)
    X = rng.standard_normal((n, d))
    return X, (X @ rng.standard_normal((d, classes)) + rng.standard_normal((n, classes))).argmax(axis=1)


def _objective_grad_norm(X, y, coef, icpt, lam):
    """‖∇‖₂ of mean loss + λ/2 ‖w‖² over the standardised columns, longdouble."""
    n = len(y)
    sig = X.astype(LD).std(axis=0, ddof=1)
    W = np.concatenate([coef.astype(LD) * sig, icpt.astype(LD)[:, None]], axis=1)
    G = _ref(X / sig, y, W, True, 0.0)[0] / n
    G[:, :-1] += lam * W[:, :-1]
    return float(np.sqrt((G * G).sum()))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("switch", [None, "0"])
def test_cpu_is_the_inline_expressions(monkeypatch, dtype, C, switch):
    if switch is not None:
        monkeypatch.setenv("SRML_LOGREG_F64", switch)
    X, y, W = (torch.from_numpy(a) for a in _data(300, 19, C, True))
    X, W = X.to(dtype), W.to(dtype)
    grad, loss = glm.logistic_grad_loss(X, y, W, True)
    resid, want = torch_ref.softmax_residual(X @ W[:, :19].T + W[:, 19][None, :], y)
    assert torch.equal(loss, want)
    assert torch.equal(grad, torch.cat([resid.T @ X, resid.sum(dim=0)[:, None]], dim=1))


@gpu
def test_65_classes_stay_f64_outside_the_kernel(ext, monkeypatch):
    def no(*a, **k):
        raise AssertionError("f64 rows reached the f32 softmax kernel")

    monkeypatch.setattr(ext, "softmax_residual_loss", no)
    X, y, W = _data(300, 129, 65, True)
    rg, rl = _ratios(_run(glm.logistic_grad_loss, X, y, W, True), X, y, W, True, C_E)
    print("worst error / bound (grad, loss)", rg, rl)
    assert rg <= 1.0 and rl <= 1.0
