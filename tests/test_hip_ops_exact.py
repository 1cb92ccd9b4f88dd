"""HIP kernels at their path boundaries, on inputs where f32 is exact.

Coordinates, weights and values are small integers held in float32, so every
product and every partial sum of a dot product, a squared distance (difference
or q²+i²−2q·i form), a Gram entry, a per-centre sum or a CSR gradient is an
integer below 2**24: exact in f32 in ANY summation order (MFMA, library GEMM,
LDS and global float atomics, splits). The kernel output must therefore equal
the int64 / float64 CPU reference exactly; ties are exact ties, so every check
is written to be invariant to tie-breaking. Each case asserts its own < 2**24
bound. Only `softmax_residual_loss` cannot be exact; its bound is derived in
the test.

The input builders and references are plain (cached) functions: the unmarked
`test_cpu_*` tests at the end run them without a GPU and show that the plain
f32 torch formulation already meets every condition the GPU tests impose.
"""

from functools import lru_cache

import numpy as np
import pytest
import torch

from spark_rapids_ml_amd.ops import torch_ref

gpu = pytest.mark.gpu
LIM = 2 ** 24


@pytest.fixture(scope="module")
def ext():
    from spark_rapids_ml_amd.ops.dispatch import hip_ops

    return hip_ops()


def _ints(rng, shape, lo, hi):
    """int64 array, uniform in [lo, hi]."""
    return rng.integers(lo, hi + 1, size=shape, dtype=np.int64)


def _nonzero_ints(rng, shape, m):
    """int64 array, uniform in [-m, m] without 0."""
    return _ints(rng, shape, 1, m) * (2 * _ints(rng, shape, 0, 1) - 1)


def _f32(a, dev="cuda"):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def _sq_dists(Q, I):
    """int64 [nq, ni] squared distances of integer rows (float64 BLAS: exact)."""
    Qd, Id = Q.astype(np.float64), I.astype(np.float64)
    D = (Qd * Qd).sum(1)[:, None] + (Id * Id).sum(1)[None, :] - 2.0 * (Qd @ Id.T)
    return D.astype(np.int64)


# ---------------------------------------------------------------------------
# 2. k-NN selection
# ---------------------------------------------------------------------------

KNN_SELECT_CASES = [
    (1, 1, 1, 1),         # smallest possible call
    (5, 64, 1, 64),       # ni == k
    (63, 127, 31, 7),     # every tail below one tile
    (65, 129, 33, 64),    # one past each tile; two item splits of 65 and 64
    (64, 384, 96, 1),     # all tiles full, unguarded staging, k=1
    (130, 999, 64, 16),   # full d-chunks, ragged item end
    (64, 16257, 8, 16),   # last item split has one item
]

KNN_GEMM_CASES = [
    (5, 513, 33, 17, 5 * 256),      # chunks of 256, 256 and 1 (< k, < a float4)
    (3, 258, 7, 64, 1 << 29),       # last chunk 2 wide: c % 4 = 2, scalar loads
    (6, 1024, 16, 63, 1 << 29),     # float4 path, c % 256 = 0, one dead slot
    (1, 64, 4, 64, 1 << 29),        # ni == k, no dead slot
    (333, 7777, 100, 1, 1 << 22),   # k=1
]


@lru_cache(maxsize=None)
def _knn_case(nq, ni, d):
    """(Q, I, D) integer queries / items in [-8, 8] and their int64 distances."""
    assert 4 * 64 * d < LIM  # (q-i)^2 <= 256 per coordinate; so is every partial sum
    rng = np.random.default_rng(1000 * nq + 10 * ni + d)
    Q, I = _ints(rng, (nq, d), -8, 8), _ints(rng, (ni, d), -8, 8)
    return Q, I, _sq_dists(Q, I)


@lru_cache(maxsize=None)
def _knn_dup_case():
    """100 distinct rows each repeated three times; queries = the first 50
    items: zero distances and ties everywhere."""
    d = 16
    assert 4 * 64 * d < LIM
    rng = np.random.default_rng(7)
    base = _ints(rng, (100, d), -8, 8)
    assert len(np.unique(base, axis=0)) == 100
    I = np.repeat(base, 3, axis=0)
    Q = I[:50].copy()
    return Q, I, _sq_dists(Q, I)


@lru_cache(maxsize=None)
def _knn_evict_case():
    """d = 1, items ni-j (descending), queries 0, 1, -3: every column improves
    tau, so each ballot carries many candidates that are stale once the first
    of them is inserted."""
    ni = 1500
    assert (ni + 3) ** 2 + ni ** 2 + 9 < LIM  # q^2 + i^2 + |2 q i| in the expansion
    I = (ni - np.arange(ni, dtype=np.int64))[:, None]
    Q = np.array([[0], [1], [-3]], dtype=np.int64)
    return Q, I, _sq_dists(Q, I)


def _check_topk(D, k, sq_vals, idx):
    """Tie-invariant top-k check of (squared values, indices) against the
    int64 distance matrix D. Returns the reference k smallest per row."""
    nq, ni = D.shape
    ref = np.sort(D, axis=1)[:, :k]
    idx = np.asarray(idx)
    assert sq_vals.shape == ref.shape and idx.shape == ref.shape
    # ascending and equal to the k smallest entries
    assert np.array_equal(np.asarray(sq_vals, dtype=np.float64), ref.astype(np.float64))
    assert idx.min() >= 0 and idx.max() < ni
    if k > 1:
        assert (np.diff(np.sort(idx, axis=1), axis=1) > 0).all(), "repeated index"
    # the distance at each reported index is the reported value
    assert np.array_equal(np.take_along_axis(D, idx.astype(np.int64), 1), ref)
    return ref


def _run_knn_select(ext, Q, I, D, k):
    d2, idx = ext.knn_select(_f32(Q), _f32(I), k)
    assert idx.dtype == torch.int64
    _check_topk(D, k, d2.cpu().numpy(), idx.cpu().numpy())


@gpu
@pytest.mark.parametrize("nq,ni,d,k", KNN_SELECT_CASES)
def test_knn_select_exact(ext, nq, ni, d, k):
    Q, I, D = _knn_case(nq, ni, d)
    if (nq, ni) == (64, 16257):
        # the wrapper's split rule: 128 item splits of 128, the last holds ONE
        # item (< k), so its (3.4e38, -1) slots reach the topk merge
        qblocks = (nq + 63) // 64
        isplit = max(1, min((ni + 127) // 128, 512 // max(1, qblocks)))
        per = (ni + isplit - 1) // isplit
        assert (isplit, per, ni - (isplit - 1) * per) == (128, 128, 1)
    if (nq, ni) == (65, 129):
        isplit = max(1, min((ni + 127) // 128, 512 // 2))
        per = (ni + isplit - 1) // isplit
        assert (isplit, per, ni - per) == (2, 65, 64)
    _run_knn_select(ext, Q, I, D, k)


@gpu
@pytest.mark.parametrize("k", [1, 7, 64])
def test_knn_select_exact_duplicates(ext, k):
    Q, I, D = _knn_dup_case()
    assert (np.sort(D, axis=1)[:, :3] == 0).all()  # each query has 3 zero distances
    _run_knn_select(ext, Q, I, D, k)


def _check_gemm_select(D, k, dd, ii):
    """`_knn_topk_gemm_select` returns sqrt'ed distances: compare with
    torch.sqrt of the exact reference on the same device."""
    ref = np.sort(D, axis=1)[:, :k]
    want = torch.sqrt(_f32(ref, dd.device))
    assert torch.equal(dd, want)
    assert ii.dtype == torch.int64
    _check_topk(D, k, ref, ii.cpu().numpy())


@gpu
@pytest.mark.parametrize("nq,ni,d,k,chunk_elems", KNN_GEMM_CASES)
def test_knn_gemm_select_exact(ext, nq, ni, d, k, chunk_elems):
    from spark_rapids_ml_amd.ops.knn import _knn_topk_gemm_select

    Q, I, D = _knn_case(nq, ni, d)
    dd, ii = _knn_topk_gemm_select(_f32(Q), _f32(I), k, chunk_elems=chunk_elems)
    _check_gemm_select(D, k, dd, ii)


@gpu
def test_knn_gemm_select_exact_eviction_stress(ext):
    from spark_rapids_ml_amd.ops.knn import _knn_topk_gemm_select

    Q, I, D = _knn_evict_case()
    for k in (1, 10, 64):
        dd, ii = _knn_topk_gemm_select(_f32(Q), _f32(I), k)
        _check_gemm_select(D, k, dd, ii)


@gpu
def test_knn_merge_topk_exact_one_258_wide_chunk(ext):
    """One call over a single [3, 258] dot block: c % 4 = 2 (scalar loads)
    and c just over one 256-column trip, which `_knn_topk_gemm_select`'s own
    chunking (multiples of 64) cannot produce."""
    nq, ni, d, k = 3, 258, 7, 64
    Q, I, D = _knn_case(nq, ni, d)
    Qt, It = _f32(Q), _f32(I)
    best_d = torch.full((nq, 64), float("inf"), device="cuda")
    best_i = torch.full((nq, 64), -1, dtype=torch.int64, device="cuda")
    G = torch.mm(Qt, It.T).contiguous()
    ext.knn_merge_topk(G, (Qt * Qt).sum(1), (It * It).sum(1), 0, best_d, best_i)
    d_sorted, order = torch.sort(best_d, dim=1)
    _check_topk(D, k, d_sorted.cpu().numpy(), best_i.gather(1, order).cpu().numpy())


@gpu
@pytest.mark.parametrize("mode", [None, "1", "0"])
def test_knn_topk_fewer_items_than_k(ext, monkeypatch, mode):
    """ni < k: every SRML_KNN_KERNEL mode returns the shape (and padding, if
    any) of `torch_ref.knn_topk`."""
    from spark_rapids_ml_amd.ops.knn import knn_topk

    if mode is None:
        monkeypatch.delenv("SRML_KNN_KERNEL", raising=False)
    else:
        monkeypatch.setenv("SRML_KNN_KERNEL", mode)
    nq, ni, d, k = 4, 3, 5, 5
    Q, I, D = _knn_case(nq, ni, d)
    ref_d, ref_i = torch_ref.knn_topk(_f32(Q, "cpu"), _f32(I, "cpu"), k)
    dd, ii = knn_topk(_f32(Q), _f32(I), k)
    assert dd.shape == ref_d.shape and ii.shape == ref_i.shape
    assert dd.dtype == ref_d.dtype and ii.dtype == ref_i.dtype
    _check_gemm_select(D, ni, dd[:, :ni].contiguous(), ii[:, :ni].contiguous())
    assert torch.equal(dd[:, ni:].cpu(), ref_d[:, ni:])
    assert torch.equal(ii[:, ni:].cpu(), ref_i[:, ni:])


# ---------------------------------------------------------------------------
# 3. gather_dists
# ---------------------------------------------------------------------------

GATHER_CASES = [(1, 1, 1, 1), (5, 7, 63, 3), (6, 50, 64, 1), (7, 50, 65, 9),
                (9, 100, 2048, 4), (1001, 300, 130, 40)]


@lru_cache(maxsize=None)
def _gather_case(r, n, d, m, same):
    """(A, B, cand, ref int64 [r, m]). same=True: B IS A (so n = r), column 0
    of every candidate list is the row itself and one candidate is repeated."""
    assert 4 * 64 * d < LIM
    rng = np.random.default_rng(17 * r + d + m + int(same))
    A = _ints(rng, (r, d), -8, 8)
    B = A if same else _ints(rng, (n, d), -8, 8)
    cand = _ints(rng, (r, m), 0, B.shape[0] - 1)
    if same:
        cand[:, 0] = np.arange(r)
        if m >= 3:
            cand[:, 2] = cand[:, 1]
    ref = ((A[:, None, :] - B[cand]) ** 2).sum(axis=2)
    return A, B, cand, ref


@gpu
@pytest.mark.parametrize("same", [False, True])
@pytest.mark.parametrize("r,n,d,m", GATHER_CASES)
def test_gather_dists_exact(ext, r, n, d, m, same):
    A, B, cand, ref = _gather_case(r, n, d, m, same)
    At = _f32(A)
    Bt = At if same else _f32(B)
    got = ext.gather_dists(At, Bt, torch.from_numpy(cand).cuda())
    if same:
        assert (ref[:, 0] == 0).all()
    assert np.array_equal(got.cpu().numpy().astype(np.float64), ref.astype(np.float64))


# ---------------------------------------------------------------------------
# 4. gram_f32
# ---------------------------------------------------------------------------

GRAM_CASES = [
    (1, 1),        # smallest call
    (63, 129),     # second block one column wide
    (64, 128),     # exactly one full block
    (65, 127),     # one row past a step, one column short of a block
    (100, 64),     # split = 64 but only 2 K-steps; most slices return early
    (777, 301),    # ragged rows and columns
    (130, 4900),   # split == 1 store path
]


@lru_cache(maxsize=None)
def _gram_case(n, d):
    assert 64 * n < LIM
    A = _ints(np.random.default_rng(n + d), (n, d), -8, 8)
    Ad = A.astype(np.float64)
    return A, (Ad.T @ Ad).astype(np.float32)  # integers < 2**24: exact in f32


@gpu
@pytest.mark.parametrize("n,d", GRAM_CASES)
def test_gram_exact(ext, n, d):
    A, ref = _gram_case(n, d)
    if d == 4900:
        nb = (d + 127) // 128
        assert nb * (nb + 1) // 2 > 768  # the wrapper's 768 // tri gives split == 1
    G = ext.gram_f32(_f32(A))
    assert torch.equal(G.cpu(), torch.from_numpy(ref))  # both triangles


# ---------------------------------------------------------------------------
# 5. label_accumulate
# ---------------------------------------------------------------------------

# (n, d, k, labels): "rand" int32, "i64" int64, "even" even ids only, "one" all equal
LABEL_CASES = [
    (3000, 128, 238, "rand"),   # LDS path at the gate
    (3000, 128, 239, "rand"),   # first size past the gate -> sort path
    (3000, 200, 50, "rand"),    # even d > 128 branch
    (3000, 126, 10, "rand"),    # idle lanes in the float2 branch
    (3000, 2, 7, "rand"),       # one float2 per row
    (1, 128, 3, "rand"),        # fewer than one 8-row group
    (7, 128, 3, "rand"),
    (513, 128, 3, "rand"),      # block tails
    (500, 4100, 8, "rand"),     # sort path, second column block
    (1000, 16, 5, "i64"),       # sort path forced by dtype
    (3000, 128, 40, "even"),    # empty clusters: zero rows, count 0
    (3000, 128, 40, "one"),     # worst skew
]


@lru_cache(maxsize=None)
def _label_case(n, d, k, kind):
    assert 8 * n < LIM
    rng = np.random.default_rng(n + 7 * d + 13 * k)
    X = _ints(rng, (n, d), -8, 8)
    if kind == "even":
        labels = 2 * _ints(rng, n, 0, (k - 1) // 2)
    elif kind == "one":
        labels = np.full(n, k - 3, dtype=np.int64)
    else:
        labels = _ints(rng, n, 0, k - 1)
    sums = torch.zeros(k, d, dtype=torch.float64)
    sums.index_add_(0, torch.from_numpy(labels), torch.from_numpy(X).double())
    counts = np.bincount(labels, minlength=k)
    return X, labels, sums.numpy(), counts


def _label_lds_bytes(d, k):
    return k * d * 4 + k * 4


@gpu
@pytest.mark.parametrize("n,d,k,kind", LABEL_CASES)
def test_label_accumulate_exact(ext, n, d, k, kind):
    X, labels, ref_sums, ref_counts = _label_case(n, d, k, kind)
    if (d, k) == (128, 238):
        assert _label_lds_bytes(d, k) == 122808 <= 120 * 1024
    if (d, k) == (128, 239):
        assert _label_lds_bytes(d, k) > 120 * 1024
    if kind == "even":
        assert (ref_counts[1::2] == 0).all() and (ref_counts[0::2] > 0).all()
    lt = torch.from_numpy(labels).to(torch.int64 if kind == "i64" else torch.int32).cuda()
    sums, counts = ext.label_accumulate(_f32(X), lt, k)
    assert sums.shape == (k, d) and counts.shape == (k,)
    assert np.array_equal(counts.cpu().numpy().astype(np.float64), ref_counts.astype(np.float64))
    assert np.array_equal(sums.cpu().numpy().astype(np.float64), ref_sums)


# ---------------------------------------------------------------------------
# 6. CSR GLM kernels
# ---------------------------------------------------------------------------


def _csr_from_dense(M):
    rows, cols = np.nonzero(M)  # row-major order
    indptr = np.zeros(M.shape[0] + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=M.shape[0]), out=indptr[1:])
    return indptr, cols.astype(np.int64), M[rows, cols]


@lru_cache(maxsize=None)
def _csr_structure_case(n, d, density):
    """Dense int64 M [n, d], about `density` non-zeros in [-4, 4]; first row,
    last row and rows 400..419 empty, row 500 holds all d columns."""
    assert 16 * max(n, d) < LIM  # |val * w| <= 16 over <= d terms / <= n rows
    rng = np.random.default_rng(n + d)
    M = _nonzero_ints(rng, (n, d), 4) * (rng.random((n, d)) < density)
    M[0] = 0
    M[n - 1] = 0
    M[400:420] = 0
    M[500] = _nonzero_ints(rng, d, 4)
    return (M,) + _csr_from_dense(M)


@lru_cache(maxsize=None)
def _csr_weights(n, d, C):
    rng = np.random.default_rng(100 + C)
    return _nonzero_ints(rng, (C, d), 4), _ints(rng, (n, C), -4, 4)


def _idx(a, dtype):
    return torch.from_numpy(a).to(dtype).cuda()


@gpu
@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("C", [1, 3, 32])
def test_csr_fwd_grad_exact_structure(ext, C, idx_dtype):
    n, d = 1000, 300
    M, indptr, indices, vals = _csr_structure_case(n, d, 0.03)
    assert indptr[1] == 0 and indptr[n] == indptr[n - 1] and indptr[501] - indptr[500] == d
    W, R = _csr_weights(n, d, C)
    ip, ix, v = _idx(indptr, idx_dtype), _idx(indices, idx_dtype), _f32(vals)
    scores = ext.csr_fwd(ip, ix, v, _f32(W.T))
    assert np.array_equal(scores.cpu().numpy().astype(np.int64), M @ W.T)
    grad = ext.csr_grad(ip, ix, v, _f32(R), d)
    assert np.array_equal(grad.cpu().numpy().astype(np.int64), R.T @ M)


@gpu
@pytest.mark.parametrize("C", [30, 31])
def test_csr_grad_exact_at_lds_gate(ext, C):
    """(C=30, d=1024) is exactly the 120 KB LDS gate; C=31 scatters to global."""
    n, d = 1000, 1024
    assert (C * d * 4 <= 120 * 1024) == (C == 30) and 30 * d * 4 == 120 * 1024
    M, indptr, indices, vals = _csr_structure_case(n, d, 0.03)
    _, R = _csr_weights(n, d, C)
    grad = ext.csr_grad(_idx(indptr, torch.int32), _idx(indices, torch.int32),
                        _f32(vals), _f32(R), d)
    assert np.array_equal(grad.cpu().numpy().astype(np.int64), R.T @ M)


@lru_cache(maxsize=None)
def _csr_stride_case():
    """n = 1 048 700 rows (> the 4096*256 one trip covers), one entry in about
    half of them. References by scatter: the dense matrix would be 0.5 GB."""
    n, d, C = 1048700, 64, 2
    assert n > 4096 * 256
    rng = np.random.default_rng(5)
    has = rng.random(n) < 0.5
    rows = np.nonzero(has)[0]
    nnz = len(rows)
    assert 16 * nnz < LIM  # even if every entry fell into one column
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(has, out=indptr[1:])
    indices = _ints(rng, nnz, 0, d - 1)
    vals = _nonzero_ints(rng, nnz, 4)
    W = _nonzero_ints(rng, (C, d), 4)
    R = _ints(rng, (n, C), -4, 4)
    scores = np.zeros((n, C), dtype=np.int64)
    scores[rows] = vals[:, None] * W[:, indices].T
    grad = np.stack([
        np.bincount(indices, weights=(vals * R[rows, c]).astype(np.float64), minlength=d)
        for c in range(C)
    ]).astype(np.int64)
    return d, indptr, indices, vals, W, R, scores, grad


@gpu
def test_csr_fwd_grad_exact_second_grid_trip(ext):
    d, indptr, indices, vals, W, R, ref_scores, ref_grad = _csr_stride_case()
    ip, ix, v = _idx(indptr, torch.int32), _idx(indices, torch.int32), _f32(vals)
    scores = ext.csr_fwd(ip, ix, v, _f32(W.T))
    assert torch.equal(scores.cpu().to(torch.int64), torch.from_numpy(ref_scores))
    assert ref_scores[4096 * 256:].any()  # the second trip has something to write
    grad = ext.csr_grad(ip, ix, v, _f32(R), d)
    assert np.array_equal(grad.cpu().numpy().astype(np.int64), ref_grad)


@lru_cache(maxsize=None)
def _csr_moments_case(d):
    nnz = 50000
    assert 16 * nnz < 2 ** 53
    rng = np.random.default_rng(d)
    indices = _ints(rng, nnz, 0, d - 1)
    indices[0], indices[1] = 0, d - 1  # both ends of the LDS table are hit
    vals = _nonzero_ints(rng, nnz, 4)
    ref = np.stack([
        np.bincount(indices, weights=vals.astype(np.float64), minlength=d),
        np.bincount(indices, weights=(vals * vals).astype(np.float64), minlength=d),
    ])
    return indices, vals, ref


@gpu
@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("d", [1, 10240])
def test_csr_col_moments_exact(ext, d, idx_dtype):
    """d = 10240 is the gate d*16 <= 160 KB of the wrapper and of
    `LogisticRegression._column_std`: the whole LDS of a CU."""
    assert 10240 * 16 == 160 * 1024
    indices, vals, ref = _csr_moments_case(d)
    mom = ext.csr_col_moments(_idx(indices, idx_dtype), _f32(vals), d)
    assert mom.dtype == torch.float64 and mom.shape == (2, d)
    assert np.array_equal(mom.cpu().numpy(), ref)


# ---------------------------------------------------------------------------
# 7. fil_predict
# ---------------------------------------------------------------------------


def _tree_from_nodes(nodes, vw):
    """nodes: list of (feature, threshold, left, right, value-or-None)."""
    m = len(nodes)
    t = {
        "feature": np.array([f for f, *_ in nodes], np.int32),
        "threshold": np.array([th for _, th, *_ in nodes], np.float32),
        "left": np.array([l for _, _, l, _, _ in nodes], np.int32),
        "right": np.array([r for _, _, _, r, _ in nodes], np.int32),
        "is_leaf": np.array([f < 0 for f, *_ in nodes], bool),
        "gain": np.zeros(m, np.float32),
        "value": np.zeros((m, vw), np.float32),
    }
    for i, node in enumerate(nodes):
        if node[4] is not None:
            t["value"][i] = node[4]
    return t


def _leaf_value(rng, classif, vw):
    if classif:  # integer counts with row sum 8 or 16: every vote is dyadic
        return rng.multinomial(int(rng.choice([8, 16])), np.full(vw, 1.0 / vw))
    return np.array([_ints(rng, (), -32, 32) / 8.0, _ints(rng, (), 1, 50)])


def _random_tree(rng, d, classif, vw, max_depth=6):
    nodes = [None]
    todo = [(0, 0)]
    while todo:
        i, depth = todo.pop()
        if depth < max_depth and (depth == 0 or rng.random() < 0.75):
            l, r = len(nodes), len(nodes) + 1
            nodes += [None, None]
            nodes[i] = (int(rng.integers(0, d)), float(rng.integers(1, 8)), l, r, None)
            todo += [(l, depth + 1), (r, depth + 1)]
        else:
            nodes[i] = (-1, 0.0, -1, -1, _leaf_value(rng, classif, vw))
    return _tree_from_nodes(nodes, vw)


@lru_cache(maxsize=None)
def _fil_forest(d, classif, vw):
    """Five random trees of depth <= 6, a stump whose root is a leaf, a
    left-only chain of depth 12 and (classification) a stump with an all-zero
    leaf, which votes 0 through the 1e-12 clamp."""
    rng = np.random.default_rng(vw + d)
    trees = [_random_tree(rng, d, classif, vw) for _ in range(5)]
    trees.append(_tree_from_nodes([(-1, 0.0, -1, -1, _leaf_value(rng, classif, vw))], vw))
    chain = []
    for lvl in range(12):  # node 2*lvl splits, 2*lvl+1 is its right leaf
        chain.append((lvl % d, float(7 - (lvl // d) % 3), 2 * lvl + 2, 2 * lvl + 1, None))
        chain.append((-1, 0.0, -1, -1, _leaf_value(rng, classif, vw)))
    chain.append((-1, 0.0, -1, -1, _leaf_value(rng, classif, vw)))
    trees.append(_tree_from_nodes(chain, vw))
    if classif:
        trees.append(_tree_from_nodes([(-1, 0.0, -1, -1, np.zeros(vw))], vw))
    return trees


def _fil_replay(X, trees, classif, vw):
    """Level-wise numpy replay; x == threshold goes RIGHT. float64 [n, vw]."""
    n = X.shape[0]
    out = np.zeros((n, vw), dtype=np.float64)
    ar = np.arange(n)
    for t in trees:
        node = np.zeros(n, dtype=np.int64)
        while not t["is_leaf"][node].all():
            leaf = t["is_leaf"][node]
            f = np.maximum(t["feature"][node], 0)
            go_left = X[ar, f] < t["threshold"][node]
            node = np.where(leaf, node, np.where(go_left, t["left"][node], t["right"][node]))
        v = t["value"][node].astype(np.float64)
        if classif:
            out += v / np.maximum(v.sum(axis=1, keepdims=True), 1e-12)
        else:
            out[:, 0] += v[:, 0]
    return out


@lru_cache(maxsize=None)
def _fil_case(n, d, classif, vw):
    """(X int64 in [0, 8), trees, ref f32 [n, vw]). Rows repeat (8**d distinct
    ones), so the replay runs on the distinct rows and is gathered."""
    trees = _fil_forest(d, classif, vw)
    X = _ints(np.random.default_rng(n), (n, d), 0, 7)
    codes = X @ (8 ** np.arange(d))
    u, inv = np.unique(codes, return_inverse=True)
    Xu = (u[:, None] // (8 ** np.arange(d))) % 8
    ref = _fil_replay(Xu.astype(np.float32), trees, classif, vw)[inv]
    assert np.array_equal(ref * 16, np.round(ref * 16))  # dyadic: exact in f32
    return X, trees, ref.astype(np.float32)


def _fil_arena(trees, dev):
    off = np.cumsum([0] + [t["feature"].shape[0] for t in trees])[:-1]
    cat = lambda key: np.concatenate([t[key] for t in trees])  # noqa: E731
    return {
        "feat": torch.from_numpy(np.where(cat("is_leaf"), -1, cat("feature")).astype(np.int32)).to(dev),
        "thr": torch.from_numpy(cat("threshold")).to(dev),
        "left": torch.from_numpy(cat("left")).to(dev),
        "right": torch.from_numpy(cat("right")).to(dev),
        "value": torch.from_numpy(cat("value")).contiguous().to(dev),
        "roots": torch.from_numpy(off.astype(np.int64)).to(dev),
    }


FIL_ROWS = [(1, 5), (255, 5), (257, 5), (4096 * 256 + 300, 3)]  # (n, d); last: second trip
FIL_KINDS = [(True, 2), (True, 16), (False, 2)]  # (classification, value width)


@gpu
@pytest.mark.parametrize("classif,vw", FIL_KINDS)
@pytest.mark.parametrize("n,d", FIL_ROWS)
def test_fil_predict_exact(ext, n, d, classif, vw):
    X, trees, ref = _fil_case(n, d, classif, vw)
    a = _fil_arena(trees, "cuda")
    out = ext.fil_predict(_f32(X), a["feat"], a["thr"], a["left"], a["right"],
                          a["value"], a["roots"], classif)
    assert torch.equal(out.cpu(), torch.from_numpy(ref))


# ---------------------------------------------------------------------------
# 8. KMeans f32 assignment paths
# ---------------------------------------------------------------------------

KM_BN = 128
KMEANS_CASES = [(1, 1, 1), (127, 63, 1), (129, 65, KM_BN + 1), (513, 200, 257)]
# second grid-stride trip: kmeans_argmin_kn caps the grid at 4096 blocks of 256
# rows, kmeans_argmin_nk at 16384 blocks of 4 rows (one wave each)
KMEANS_STRIDE = {"kn": (4096 * 256 + 300, 4, 3), "nk": (16384 * 4 + 5, 4, 3)}


@lru_cache(maxsize=None)
def _kmeans_case(n, d, k):
    """(X, C, D int64 [n, k]); every third centre repeats its predecessor, so
    exact ties exist."""
    assert 4 * 64 * d < LIM
    rng = np.random.default_rng(n + d + k)
    X, C = _ints(rng, (n, d), -8, 8), _ints(rng, (k, d), -8, 8)
    C[2::3] = C[1::3][: len(C[2::3])]
    X[: min(n, k)] = C[: min(n, k)]  # zero distances too
    return X, C, _sq_dists(X, C)


def _check_assign(D, labels, inertia, min_d=None):
    rowmin = D.min(axis=1)
    lab = labels.cpu().numpy().astype(np.int64)
    assert lab.shape == rowmin.shape and lab.min() >= 0 and lab.max() < D.shape[1]
    assert np.array_equal(D[np.arange(len(lab)), lab], rowmin)
    if min_d is not None:
        assert np.array_equal(min_d.cpu().numpy().astype(np.float64), rowmin.astype(np.float64))
    assert inertia.dtype == torch.float64
    assert float(inertia.item()) == float(rowmin.sum())


def _argmin_direct(ext, Xt, Ct, layout):
    """The epilogue kernels on a whole dot block: they return min_d, which
    `_assign_gemm` drops."""
    x_sq, c_sq = (Xt * Xt).sum(1).contiguous(), (Ct * Ct).sum(1).contiguous()
    if layout == "kn":
        return ext.kmeans_argmin_kn(torch.mm(Ct, Xt.T).contiguous(), x_sq, c_sq)
    return ext.kmeans_argmin_nk(torch.mm(Xt, Ct.T).contiguous(), x_sq, c_sq)


@gpu
@pytest.mark.parametrize("n,d,k", KMEANS_CASES)
def test_kmeans_assign_fused_exact(ext, n, d, k):
    X, C, D = _kmeans_case(n, d, k)
    Xt, Ct = _f32(X), _f32(C)
    labels, min_d, inertia = ext.kmeans_assign(Xt, Ct, (Xt * Xt).sum(1))
    assert labels.dtype == torch.int32
    _check_assign(D, labels, inertia, min_d)


@gpu
@pytest.mark.parametrize("layout", ["kn", "nk"])
@pytest.mark.parametrize("case", KMEANS_CASES + ["stride"], ids=str)
def test_kmeans_assign_gemm_exact(ext, case, layout):
    from spark_rapids_ml_amd.ops.kmeans import _assign_gemm

    n, d, k = KMEANS_STRIDE[layout] if case == "stride" else case
    X, C, D = _kmeans_case(n, d, k)
    Xt, Ct = _f32(X), _f32(C)
    x_sq = (Xt * Xt).sum(1)
    labels, inertia = _assign_gemm(ext, Xt, Ct, x_sq, n, k, layout=layout)
    _check_assign(D, labels, inertia)
    labels, min_d, inertia = _argmin_direct(ext, Xt, Ct, layout)
    _check_assign(D, labels, inertia, min_d)


# ---------------------------------------------------------------------------
# 9. softmax_residual_loss (cannot be exact)
# ---------------------------------------------------------------------------

# Residual bound, absolute per element. __expf(x) is exp2(x*log2e): rounding
# the argument gives a relative error of about |x|*2^-24 plus one ulp of the
# exp2; p = e^-|x| weights that error and |x|e^-|x| <= 0.37; the denominator
# carries the same class of error and the division a few ulp: <~ 20 * 2^-24.
RESID_BOUND = 32 * 2.0 ** -24
LOSS_RTOL = 1e-4  # the project's existing tolerance, now against float64

# (n, C, all labels equal); 524365 = 2048*256 + 77 reaches the second trip
SOFTMAX_CASES = [(1, 1, False), (63, 1, False), (524365, 1, False), (524365, 3, False),
                 (513, 2, False), (513, 17, False), (300, 40, False),
                 (63, 1, True), (513, 17, True)]


@lru_cache(maxsize=None)
def _softmax_case(n, C, one_label):
    """(scores f32 [n, C], y int64, ref resid f64, ref loss f64)."""
    g = torch.Generator().manual_seed(n + C)
    scores = torch.randn(n, C, generator=g, dtype=torch.float32) * 10
    if C == 1:
        planted = torch.tensor([0.0, 20.0, -20.0, 100.0, -100.0])[:, None]
    else:
        planted = torch.stack([torch.full((C,), 3.0), torch.full((C,), 80.0),
                               torch.full((C,), -88.0)])
        planted[2, C // 2] = 88.0
    m = min(n, planted.shape[0])
    scores[:m] = planted[:m]
    y = torch.randint(0, max(2, C), (n,), generator=g)
    if one_label:
        y = torch.full((n,), max(2, C) - 1, dtype=torch.int64)
    s64 = scores.double()
    if C == 1:
        z, yd = s64[:, 0], y.double()
        ref = (torch.sigmoid(z) - yd)[:, None]
        loss = torch.nn.functional.softplus(-(2 * yd - 1) * z).sum()
    else:
        logp = torch.log_softmax(s64, dim=1)
        ref = torch.exp(logp)
        ref[torch.arange(n), y] -= 1.0
        loss = -logp[torch.arange(n), y].sum()
    return scores, y, ref, float(loss)


def _check_softmax(resid, loss, y, ref, ref_loss, C):
    """resid f32 [n, C] and loss (0-dim) on the CPU. Returns the measured
    (max residual error, relative loss error)."""
    assert torch.isfinite(resid).all() and torch.isfinite(loss).all()
    r = resid.double()
    err = float((r - ref).abs().max())
    rel = abs(float(loss) - ref_loss) / abs(ref_loss)
    print(f"softmax n={len(y)} C={C}: max|resid-ref|={err:.3e} (bound {RESID_BOUND:.3e}) "
          f"loss rel err={rel:.3e} (bound {LOSS_RTOL:.0e})")
    assert err <= RESID_BOUND
    assert rel <= LOSS_RTOL
    hot = torch.zeros_like(r, dtype=torch.bool)
    if C == 1:
        hot[:, 0] = y == 1
    else:
        hot[torch.arange(len(y)), y] = True
        assert float(r.sum(dim=1).abs().max()) <= C * RESID_BOUND
    assert (r[hot] >= -1.0).all() and (r[hot] <= 0.0).all()
    assert (r[~hot] >= 0.0).all() and (r[~hot] <= 1.0).all()
    return err, rel


@gpu
@pytest.mark.parametrize("n,C,one_label", SOFTMAX_CASES)
def test_softmax_residual_within_derived_bound(ext, n, C, one_label):
    scores, y, ref, ref_loss = _softmax_case(n, C, one_label)
    resid, loss = ext.softmax_residual_loss(scores.cuda(), y.cuda())
    assert resid.shape == (n, C)
    _check_softmax(resid.cpu(), loss.cpu(), y, ref, ref_loss, C)


# ---------------------------------------------------------------------------
# 10. CPU preconditions: the plain f32 torch formulation on the same inputs
# already equals the integer reference (and, for softmax, sits inside the bound)
# ---------------------------------------------------------------------------


def _f32_expansion(Q, I):
    Qt, It = _f32(Q, "cpu"), _f32(I, "cpu")
    return (Qt * Qt).sum(1)[:, None] + (It * It).sum(1)[None, :] - 2.0 * (Qt @ It.T)


def test_cpu_knn_inputs_exact_in_f32():
    cases = [_knn_case(nq, ni, d) for nq, ni, d, _ in KNN_SELECT_CASES]
    cases += [_knn_case(nq, ni, d) for nq, ni, d, _, _ in KNN_GEMM_CASES]
    cases += [_knn_dup_case(), _knn_evict_case(), _knn_case(4, 3, 5)]
    for Q, I, D in cases:
        assert 0 <= D.min() and D.max() < LIM
        assert torch.equal(_f32_expansion(Q, I).to(torch.int64), torch.from_numpy(D))
        # the reference passes its own check
        k = min(7, I.shape[0])
        order = np.argsort(D, axis=1, kind="stable")[:, :k]
        _check_topk(D, k, np.take_along_axis(D, order, 1), order)


def test_cpu_gather_inputs_exact_in_f32():
    for r, n, d, m in GATHER_CASES:
        for same in (False, True):
            A, B, cand, ref = _gather_case(r, n, d, m, same)
            assert ref.max() < LIM and cand.min() >= 0 and cand.max() < B.shape[0]
            got = ((_f32(A, "cpu")[:, None, :] - _f32(B, "cpu")[cand]) ** 2).sum(dim=2)
            assert torch.equal(got.to(torch.int64), torch.from_numpy(ref))


def test_cpu_gram_inputs_exact_in_f32():
    for n, d in GRAM_CASES:
        A, ref = _gram_case(n, d)
        assert np.abs(ref).max() < LIM
        At = _f32(A, "cpu")
        assert torch.equal(At.T @ At, torch.from_numpy(ref))
        assert np.array_equal(ref, ref.T)


def test_cpu_label_accumulate_inputs_exact_in_f32():
    for n, d, k, kind in LABEL_CASES:
        X, labels, ref_sums, ref_counts = _label_case(n, d, k, kind)
        assert np.abs(ref_sums).max() < LIM and ref_counts.sum() == n
        assert labels.min() >= 0 and labels.max() < k
        sums = torch.zeros(k, d).index_add_(0, torch.from_numpy(labels), _f32(X, "cpu"))
        assert np.array_equal(sums.numpy().astype(np.float64), ref_sums)


def test_cpu_csr_inputs_exact_in_f32():
    for n, d, Cs in [(1000, 300, (1, 3, 32)), (1000, 1024, (30, 31))]:
        M, indptr, indices, vals = _csr_structure_case(n, d, 0.03)
        assert indices.min() >= 0 and indices.max() < d and (vals != 0).all()
        assert indptr[-1] == len(vals) == np.count_nonzero(M)
        assert 0.02 < len(vals) / (n * d) < 0.04
        for C in Cs:
            W, R = _csr_weights(n, d, C)
            Mt = _f32(M, "cpu")
            assert np.abs(M @ W.T).max() < LIM and np.abs(R.T @ M).max() < LIM
            assert torch.equal((Mt @ _f32(W, "cpu").T).to(torch.int64), torch.from_numpy(M @ W.T))
            assert torch.equal((_f32(R, "cpu").T @ Mt).to(torch.int64), torch.from_numpy(R.T @ M))
    d, indptr, indices, vals, W, R, scores, grad = _csr_stride_case()
    assert indices.max() < d and indptr[-1] == len(vals) and np.diff(indptr).max() == 1
    assert np.abs(scores).max() <= 16 and np.abs(grad).max() < LIM
    g32 = torch.zeros(d).index_add_(
        0, torch.from_numpy(indices), _f32(vals * R[np.diff(indptr) == 1, 0], "cpu"))
    assert torch.equal(g32.to(torch.int64), torch.from_numpy(grad[0]))
    for dm in (1, 10240):
        indices, vals, ref = _csr_moments_case(dm)
        assert indices.max() == dm - 1 and np.array_equal(ref, np.round(ref))
        assert ref[1].sum() == (vals * vals).sum()


@pytest.mark.parametrize("classif,vw", FIL_KINDS)
def test_cpu_forest_traverse_matches_replay(classif, vw):
    """`ops.forest.forest_traverse` on the same dictionaries, on the CPU."""
    from spark_rapids_ml_amd.ops.forest import forest_traverse

    for n, d in FIL_ROWS[:3]:
        X, trees, ref = _fil_case(n, d, classif, vw)
        a = _fil_arena(trees, "cpu")
        assert int(a["roots"][-1]) + trees[-1]["feature"].shape[0] == a["feat"].shape[0]
        for t in trees:  # every child id stays inside its tree
            inner = ~t["is_leaf"]
            m = t["feature"].shape[0]
            assert (t["left"][inner] < m).all() and (t["right"][inner] < m).all()
            assert (t["left"][inner] > 0).all() and (t["right"][inner] > 0).all()
            assert (t["feature"][inner] < d).all()
        task = "classification" if classif else "regression"
        got = forest_traverse(_f32(X, "cpu"), trees, task, vw)
        want = torch.from_numpy(ref) if classif else torch.from_numpy(ref[:, 0])
        assert torch.equal(got, want)
    # x == threshold occurs and goes right: a one-split tree says so directly
    t = _tree_from_nodes([(0, 3.0, 1, 2, None), (-1, 0.0, -1, -1, [1.0, 0.0]),
                          (-1, 0.0, -1, -1, [0.0, 1.0])], 2)
    out = _fil_replay(np.array([[2.0], [3.0], [4.0]], np.float32), [t], True, 2)
    assert np.array_equal(out, [[1, 0], [0, 1], [0, 1]])


def test_cpu_kmeans_inputs_exact_in_f32():
    for n, d, k in KMEANS_CASES + list(KMEANS_STRIDE.values()):
        X, C, D = _kmeans_case(n, d, k)
        assert 0 <= D.min() and D.max() < LIM
        assert torch.equal(_f32_expansion(X, C).to(torch.int64), torch.from_numpy(D))
        if k >= 3:
            assert np.array_equal(C[1], C[2])  # exact ties exist
    assert KMEANS_STRIDE["kn"][0] > 4096 * 256 and KMEANS_STRIDE["nk"][0] > 16384 * 4


@pytest.mark.parametrize("n,C,one_label", SOFTMAX_CASES)
def test_cpu_softmax_f32_reference_within_bound(n, C, one_label):
    scores, y, ref, ref_loss = _softmax_case(n, C, one_label)
    resid, loss = torch_ref.softmax_residual(scores, y)
    _check_softmax(resid, loss, y, ref, ref_loss, C)
