"""kNN under the non-euclidean metrics: the `pairwise_dist` tile kernel, the
key top-k merge and the GEMM-family reductions behind `knn_topk_metric`.

Three kinds of check, each with a plain (cached) input builder and reference:

* exact — integer coordinates in [-8, 8] held in f32: every L1 sum, Linf
  maximum and hamming count is an integer far below 2**24, exact in f32 in any
  summation order, so the kernel must reproduce the int64 reference bit for
  bit. Ties are exact ties; every comparison is invariant to tie-breaking.
* bounded — minkowski (p = 3, 1.5) and canberra against scipy `cdist` in f64.
  All terms are non-negative (no cancellation); the relative bound is derived
  in `_lp_bound` / `_canberra_bound` from the term count and the documented
  ulp error of the instructions used, not from any output.
* GEMM family — cosine, correlation, hellinger against scipy / the f64
  formula with an absolute bound derived from d for a unit-row dot product.

The unmarked `test_cpu_*` tests run the same builders and checks on the CPU
(`torch_ref`), showing the plain f32 torch formulation meets every condition
the GPU tests impose.
"""

from functools import lru_cache

import numpy as np
import pytest
import torch
from scipy.spatial.distance import cdist

from spark_rapids_ml_amd.ops import knn as knn_ops
from spark_rapids_ml_amd.ops import torch_ref
from spark_rapids_ml_amd.ops.knn import knn_topk, knn_topk_metric, resolve_metric

gpu = pytest.mark.gpu
LIM = 2 ** 24
U = 2.0 ** -24  # f32 unit roundoff; 1 ulp <= 2 U relative

# (nq, ni, d, k, chunk_elems)
CASES = [
    (1, 1, 1, 1, 1 << 29),          # smallest possible call
    (5, 64, 1, 64, 1 << 29),        # ni == k, no dead slot
    (63, 127, 31, 7, 1 << 29),      # every tail below one tile
    (129, 129, 33, 64, 1 << 29),    # one past each tile and d-chunk
    (128, 384, 64, 1, 1 << 29),     # all tiles full, k = 1
    (3, 258, 7, 17, 3 * 256),       # chunks of 256 and 2: scalar-load tail of the merge
    (130, 999, 130, 16, 130 * 256), # ragged everything, 9 d-chunks, 4 item chunks
]
EXACT_METRICS = ["manhattan", "chebyshev", "hamming"]
SCIPY_NAME = {"manhattan": "cityblock"}


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


# ---------------------------------------------------------------------------
# builders and references
# ---------------------------------------------------------------------------


def _int_keys(Q, I, metric):
    """int64 [nq, ni] keys of integer rows: L1 sum, Linf max, mismatch count."""
    D = np.zeros((Q.shape[0], I.shape[0]), dtype=np.int64)
    for t in range(Q.shape[1]):
        q, x = Q[:, t, None], I[None, :, t]
        if metric == "manhattan":
            D += np.abs(q - x)
        elif metric == "chebyshev":
            D = np.maximum(D, np.abs(q - x))
        else:
            D += q != x
    return D


@lru_cache(maxsize=None)
def _int_case(nq, ni, d):
    assert 16 * d < LIM  # |q-i| <= 16 per coordinate, so is every partial sum
    rng = np.random.default_rng(1000 * nq + 10 * ni + d)
    Q = rng.integers(-8, 9, size=(nq, d), dtype=np.int64)
    I = rng.integers(-8, 9, size=(ni, d), dtype=np.int64)
    return Q, I, {m: _int_keys(Q, I, m) for m in EXACT_METRICS}


@lru_cache(maxsize=None)
def _dup_case():
    """100 distinct rows each repeated three times; queries = the first 50
    items: zero distances and ties everywhere."""
    d = 16
    rng = np.random.default_rng(7)
    base = rng.integers(-8, 9, size=(100, d), dtype=np.int64)
    assert len(np.unique(base, axis=0)) == 100
    I = np.repeat(base, 3, axis=0)
    Q = I[:50].copy()
    return Q, I, {m: _int_keys(Q, I, m) for m in EXACT_METRICS}


@lru_cache(maxsize=None)
def _real_case(nq, ni, d, zeros):
    """Continuous f32 rows. With `zeros`, a fifth of the entries on each side
    is 0, so both sides are 0 at the same coordinate for many pairs."""
    rng = np.random.default_rng(77 + 1000 * nq + 10 * ni + d)
    Q = rng.normal(size=(nq, d)).astype(np.float32)
    I = rng.normal(size=(ni, d)).astype(np.float32)
    if zeros:
        Q[rng.random(Q.shape) < 0.2] = 0.0
        I[rng.random(I.shape) < 0.2] = 0.0
        Q[0, 0] = I[0, 0] = 0.0  # both sides 0 at one coordinate: a 0/0 term
    return Q, I


def _diff_log_range(Q, I):
    """max |log2 |q - x|| over all pairs and coordinates with q != x (f64)."""
    lo, hi = np.inf, 0.0
    for t in range(Q.shape[1]):
        a = np.abs(Q[:, t, None].astype(np.float64) - I[None, :, t].astype(np.float64))
        nz = a[a > 0]
        if nz.size:
            lo, hi = min(lo, nz.min()), max(hi, nz.max())
    return max(abs(np.log2(lo)), abs(np.log2(hi)))


def _gamma(n):
    return n * U / (1.0 - n * U)


def _lp_bound(Q, I, p):
    """Relative bound on the minkowski distance.

    Per term |q-x|^p = exp2(p * log2 |q-x|) with v_log_f32 / v_exp_f32, both
    documented at 1 ulp (<= 2U relative):
      fl(q-x)            : relative U, raised to p        -> p U
      log2               : <= 2U relative on L = log2|.|
      p * L              : U relative                     -> |E| 3U absolute on E = pL,
                           i.e. ln2 * 3U * |E| relative on 2^E
      exp2               : 2U
    The d non-negative terms are summed in f32 in some order: gamma_d. The host
    takes key^(1/p): the key's error shrinks by 1/p, and pow is given 2 ulp.
    |E| <= p * max |log2|q-x|| is a property of the inputs, computed in f64."""
    d = Q.shape[1]
    e_max = p * _diff_log_range(Q, I)
    term = p * U + np.log(2.0) * 3 * U * e_max + 2 * U
    return (term + _gamma(d)) / p + 4 * U


def _canberra_bound(d):
    """fl(q-x), fl(|q|+|x|), v_rcp_f32 (1 ulp = 2U), the product: 5U per term,
    gamma_d for the f32 sum of d non-negative terms, U for the final rounding
    against the f64 reference."""
    return _gamma(d + 6)


# ---------------------------------------------------------------------------
# tie-invariant checks
# ---------------------------------------------------------------------------


def _check_indices(idx, ni, k):
    assert idx.dtype == np.int64 and idx.shape[1] == k
    assert idx.min() >= 0 and idx.max() < ni
    if k > 1:
        assert (np.diff(np.sort(idx, axis=1), axis=1) > 0).all(), "repeated index"


def _check_exact(D, k, metric, d, dists, idx):
    """Sorted k distances equal the reference's; the true distance at each
    returned index equals the returned distance."""
    dists, idx = dists.cpu().numpy(), idx.cpu().numpy()
    _check_indices(idx, D.shape[1], k)
    ref = np.sort(D, axis=1)[:, :k].astype(np.float32)
    at = np.take_along_axis(D, idx, 1).astype(np.float32)
    if metric == "hamming":  # one correctly rounded f32 division of the exact count
        ref, at = ref / np.float32(d), at / np.float32(d)
    assert dists.dtype == np.float32
    assert np.array_equal(dists, ref)
    assert np.array_equal(at, dists)


def _check_close(D, k, dists, idx, rel=0.0, abs_=0.0):
    """As _check_exact within |got - ref| <= rel * ref + abs_ (D in f64).
    An entrywise perturbation of the distances by at most that much moves each
    order statistic by at most that much."""
    dists, idx = dists.cpu().numpy().astype(np.float64), idx.cpu().numpy()
    _check_indices(idx, D.shape[1], k)
    assert (np.diff(dists, axis=1) >= 0).all()
    ref = np.sort(D, axis=1)[:, :k]
    at = np.take_along_axis(D, idx, 1)
    for want in (ref, at):
        err = np.abs(dists - want)
        tol = rel * want + abs_
        assert (err <= tol).all(), (float((err - tol).max()), float(err.max()))


def _run_exact(dev, case, k, metric, chunk_elems=1 << 29):
    Q, I, keys = case
    dists, idx = knn_topk_metric(_t(Q, dev), _t(I, dev), k, metric, chunk_elems=chunk_elems)
    _check_exact(keys[metric], k, metric, Q.shape[1], dists, idx)


def _run_bounded(dev, nq, ni, d, k, chunk_elems, metric, p=2.0):
    Q, I = _real_case(nq, ni, d, metric == "canberra")
    Q64, I64 = Q.astype(np.float64), I.astype(np.float64)
    if metric == "minkowski":
        D, rel = cdist(Q64, I64, "minkowski", p=p), _lp_bound(Q, I, p)
    else:
        D, rel = cdist(Q64, I64, "canberra"), _canberra_bound(d)
    assert rel < 1e-4  # a bound this derivation keeps meaningful
    dists, idx = knn_topk_metric(_t(Q, dev), _t(I, dev), k, metric, p=p, chunk_elems=chunk_elems)
    _check_close(D, k, dists, idx, rel=rel)


# --- GEMM family -----------------------------------------------------------


@lru_cache(maxsize=None)
def _gemm_case(metric, nq=130, ni=999, d=33):
    """(Q, I, D f64, absolute bound).

    Unit row x' = x / sqrt(sum x^2): gamma_{d+1}/2 + 2U relative per element
    (sum of squares, sqrt, division) =: e. The dot of two unit rows has
    sum |x'_i y'_i| <= 1, so any-order f32 accumulation errs by gamma_d and the
    input perturbations by 2e; 1 - dot adds 2U: (2d + 7) U after rounding up.
    correlation: the f32 row mean errs by gamma_d * mean|x|, a common shift
    of every coordinate, i.e. a vector of norm gamma_d mean|x| sqrt(d) added to
    a centred row of norm ||x - mean||: kappa = max over rows of that ratio
    (f64, from the inputs) enters twice. hellinger rows are normalised to sum
    1, so sqrt rows are unit rows up to rounding; sqrt is given 1 ulp: dot
    errs by gamma_d + 4U, 1 - dot by U more; compared on the squared distance
    (the sqrt's own ulp is 4U relative there)."""
    rng = np.random.default_rng(5)
    if metric == "hellinger":
        Q = rng.random((nq, d)) + 0.01
        I = rng.random((ni, d)) + 0.01
        Q = (Q / Q.sum(1, keepdims=True)).astype(np.float32)
        I = (I / I.sum(1, keepdims=True)).astype(np.float32)
        D = 1.0 - np.sqrt(Q.astype(np.float64)) @ np.sqrt(I.astype(np.float64)).T
        return Q, I, np.maximum(D, 0.0), (d + 5) * U  # D is the SQUARED distance
    Q = rng.normal(size=(nq, d)).astype(np.float32)
    I = rng.normal(size=(ni, d)).astype(np.float32)
    D = cdist(Q.astype(np.float64), I.astype(np.float64), metric)
    bound = (2 * d + 7) * U
    if metric == "correlation":
        A = np.concatenate([Q, I]).astype(np.float64)
        kappa = (np.abs(A).mean(1) * np.sqrt(d) / np.linalg.norm(A - A.mean(1, keepdims=True), axis=1)).max()
        bound += 2 * _gamma(d) * kappa
    return Q, I, D, bound


def _run_gemm(dev, metric, k=16):
    Q, I, D, bound = _gemm_case(metric)
    dists, idx = knn_topk_metric(_t(Q, dev), _t(I, dev), k, metric)
    if metric == "hellinger":
        _check_close(D, k, dists.to(torch.float64) ** 2, idx, rel=4 * U, abs_=bound)
    else:
        _check_close(D, k, dists, idx, abs_=bound)


def _run_cosine_pow2(dev):
    """Scaling each row by its own 2^j scales its norm by exactly 2^j and the
    division is exact: identical unit rows, identical results."""
    Q, I, _, _ = _gemm_case("cosine")
    rng = np.random.default_rng(9)
    sq = (2.0 ** rng.integers(-3, 4, size=(Q.shape[0], 1))).astype(np.float32)
    si = (2.0 ** rng.integers(-3, 4, size=(I.shape[0], 1))).astype(np.float32)
    d0, i0 = knn_topk_metric(_t(Q, dev), _t(I, dev), 16, "cosine")
    d1, i1 = knn_topk_metric(_t(Q * sq, dev), _t(I * si, dev), 16, "cosine")
    assert torch.equal(d0, d1) and torch.equal(i0, i1)


def _run_raises(dev):
    Q, I, _, _ = _gemm_case("cosine")
    Z = I.copy()
    Z[3] = 0.0
    with pytest.raises(ValueError, match="zero-norm"):
        knn_topk_metric(_t(Q, dev), _t(Z, dev), 5, "cosine")
    Z[3] = 2.5
    with pytest.raises(ValueError, match="constant"):
        knn_topk_metric(_t(Q, dev), _t(Z, dev), 5, "correlation")
    N = np.abs(I)
    N[3, 1] = -0.25
    with pytest.raises(ValueError, match="non-negative"):
        knn_topk_metric(_t(np.abs(Q), dev), _t(N, dev), 5, "hellinger")


def _run_euclidean_is_knn_topk(dev):
    Q, I = _real_case(63, 127, 31, False)
    want = knn_topk(_t(Q, dev), _t(I, dev), 7)
    for metric, p in (("euclidean", 2.0), ("l2", 2.0), ("minkowski", 2.0)):
        got = knn_topk_metric(_t(Q, dev), _t(I, dev), 7, metric, p=p)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    sq = knn_topk_metric(_t(Q, dev), _t(I, dev), 7, "sqeuclidean")
    D = cdist(Q.astype(np.float64), I.astype(np.float64), "sqeuclidean")
    # q^2 + i^2 - 2 q.i: three sums of d products around |q|^2 + |i|^2
    mag = (Q.astype(np.float64) ** 2).sum(1).max() + (I.astype(np.float64) ** 2).sum(1).max()
    _check_close(D, 7, sq[0], sq[1], abs_=2 * _gamma(31 + 2) * mag)


# ---------------------------------------------------------------------------
# the resolver (no device)
# ---------------------------------------------------------------------------


def test_resolve_metric_aliases_and_errors():
    names = "l1 cityblock taxicab manhattan euclidean l2 sqeuclidean canberra minkowski " \
            "chebyshev linf cosine correlation hellinger hamming".split()
    canon = {"l1": "manhattan", "cityblock": "manhattan", "taxicab": "manhattan",
             "l2": "euclidean", "linf": "chebyshev", "minkowski": "euclidean"}
    for n in names:
        assert resolve_metric(n)[0] == canon.get(n, n)
    assert resolve_metric("minkowski", 1) == ("manhattan", 2.0)
    assert resolve_metric("minkowski", 3) == ("minkowski", 3.0)
    assert resolve_metric("Cosine")[0] == "cosine"
    with pytest.raises(ValueError, match="Metric 'jaccard' not supported for dense inputs."):
        resolve_metric("jaccard")
    with pytest.raises(ValueError, match="canberra.*taxicab"):
        resolve_metric("mahalanobis")
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="finite and > 0"):
            resolve_metric("minkowski", bad)


def test_cpu_pairwise_distances_match_scipy():
    Q, I = _real_case(63, 127, 31, True)
    for metric in ("manhattan", "chebyshev", "canberra", "hamming", "cosine", "correlation",
                   "sqeuclidean", "euclidean"):
        D = cdist(Q.astype(np.float64), I.astype(np.float64), SCIPY_NAME.get(metric, metric))
        got = torch_ref.pairwise_distances(_t(Q, "cpu"), _t(I, "cpu"), metric).numpy()
        assert np.allclose(got, D, rtol=1e-5, atol=1e-5), metric
    D = cdist(Q.astype(np.float64), I.astype(np.float64), "minkowski", p=3)
    got = torch_ref.pairwise_distances(_t(Q, "cpu"), _t(I, "cpu"), "minkowski", 3.0).numpy()
    assert np.allclose(got, D, rtol=1e-5)


# ---------------------------------------------------------------------------
# CPU runs of every check (torch_ref)
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("metric", EXACT_METRICS)
@pytest.mark.parametrize("nq,ni,d,k,chunk_elems", CASES)
def test_cpu_exact(nq, ni, d, k, chunk_elems, metric):
    _run_exact("cpu", _int_case(nq, ni, d), k, metric, chunk_elems)


@pytest.mark.parametrize("metric", EXACT_METRICS)
def test_cpu_exact_duplicates(metric):
    _run_exact("cpu", _dup_case(), 10, metric)


@pytest.mark.parametrize("metric,p", [("minkowski", 3.0), ("minkowski", 1.5), ("canberra", 2.0)])
@pytest.mark.parametrize("nq,ni,d,k,chunk_elems", CASES[1:])
def test_cpu_bounded(nq, ni, d, k, chunk_elems, metric, p):
    _run_bounded("cpu", nq, ni, d, k, chunk_elems, metric, p)


@pytest.mark.parametrize("metric", ["cosine", "correlation", "hellinger"])
def test_cpu_gemm_family(metric):
    _run_gemm("cpu", metric)


def test_cpu_cosine_power_of_two_row_scales():
    _run_cosine_pow2("cpu")


def test_cpu_undefined_rows_raise():
    _run_raises("cpu")


def test_cpu_euclidean_is_knn_topk():
    _run_euclidean_is_knn_topk("cpu")


def test_cpu_k_above_64():
    _run_exact("cpu", _int_case(63, 127, 31), 70, "manhattan")


# ---------------------------------------------------------------------------
# GPU: the kernels
# ---------------------------------------------------------------------------


@pytest.fixture
def kernel_only(monkeypatch):
    """The torch path must not be what answers on the GPU."""

    def _no(*a, **k):
        raise AssertionError("torch fallback taken on the GPU")

    monkeypatch.setattr(torch_ref, "knn_topk_metric", _no)


@gpu
@pytest.mark.parametrize("op,metric", [(0, "manhattan"), (1, "chebyshev"), (4, "hamming")])
@pytest.mark.parametrize("nq,ni,d,k,chunk_elems", CASES)
def test_pairwise_dist_block_exact(nq, ni, d, k, chunk_elems, op, metric):
    """The whole [nq, ni] key block, not only its k smallest entries."""
    from spark_rapids_ml_amd.ops.dispatch import hip_ops

    Q, I, keys = _int_case(nq, ni, d)
    out = torch.full((nq, ni), -1.0, dtype=torch.float32, device="cuda")
    hip_ops().pairwise_dist(_t(Q, "cuda"), _t(I, "cuda"), op, 2.0, out)
    assert np.array_equal(out.cpu().numpy().astype(np.int64), keys[metric])


@gpu
@pytest.mark.parametrize("metric", EXACT_METRICS)
@pytest.mark.parametrize("nq,ni,d,k,chunk_elems", CASES)
def test_exact(nq, ni, d, k, chunk_elems, metric, kernel_only):
    _run_exact("cuda", _int_case(nq, ni, d), k, metric, chunk_elems)


@gpu
@pytest.mark.parametrize("metric", EXACT_METRICS)
def test_exact_duplicates(metric, kernel_only):
    _run_exact("cuda", _dup_case(), 10, metric)


@gpu
@pytest.mark.parametrize("metric,p", [("minkowski", 3.0), ("minkowski", 1.5), ("canberra", 2.0)])
@pytest.mark.parametrize("nq,ni,d,k,chunk_elems", CASES[1:])
def test_bounded(nq, ni, d, k, chunk_elems, metric, p, kernel_only):
    _run_bounded("cuda", nq, ni, d, k, chunk_elems, metric, p)


@gpu
@pytest.mark.parametrize("metric", ["cosine", "correlation", "hellinger"])
def test_gemm_family(metric, kernel_only):
    _run_gemm("cuda", metric)


@gpu
def test_cosine_power_of_two_row_scales(kernel_only):
    _run_cosine_pow2("cuda")


@gpu
def test_undefined_rows_raise():
    _run_raises("cuda")


@gpu
def test_euclidean_is_knn_topk(kernel_only):
    _run_euclidean_is_knn_topk("cuda")


@gpu
def test_k_above_64_takes_torch_path():
    _run_exact("cuda", _int_case(63, 127, 31), 70, "manhattan")


@gpu
def test_binding_checks():
    from spark_rapids_ml_amd.ops.dispatch import hip_ops

    ext = hip_ops()
    Q = torch.zeros((4, 3), device="cuda")
    I = torch.zeros((5, 3), device="cuda")
    out = torch.zeros((4, 5), device="cuda")
    best_d = torch.zeros((4, 64), device="cuda")
    best_i = torch.zeros((4, 64), dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError):
        ext.pairwise_dist(Q, torch.zeros((5, 4), device="cuda"), 0, 2.0, out)
    with pytest.raises(RuntimeError):
        ext.pairwise_dist(Q, I, 7, 2.0, out)
    with pytest.raises(RuntimeError):
        ext.pairwise_dist(Q.double(), I, 0, 2.0, out)
    with pytest.raises(RuntimeError):
        ext.pairwise_dist(Q, I, 2, 0.0, out)
    with pytest.raises(RuntimeError):
        ext.pairwise_dist(Q.cpu(), I, 0, 2.0, out)
    with pytest.raises(RuntimeError):
        ext.knn_merge_topk_keys(out, 0, best_d[:, :32], best_i)
    with pytest.raises(RuntimeError):
        ext.knn_merge_topk_keys(out.t(), 0, best_d, best_i)
    assert knn_ops.TILE_OPS["hamming"] == 4
