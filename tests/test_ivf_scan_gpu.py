"""GPU: the fused `ivf_scan_topk` kernel against the torch scan on the same
device tensors, then the new ANN metrics and cosine DBSCAN end to end on the
device."""

import numpy as np
import pytest
import torch

from spark_rapids_ml_amd.models import knn as knn_mod
from tests.test_ann_metrics import NEW_METRICS, _data, _kneighbors, assert_exact
from tests.test_dbscan_cosine import check_against_sklearn, cosine_fixture

pytestmark = pytest.mark.gpu

N, NLIST = 3000, 7
# list 0 empty, list 1 a single row, list 2 shorter than k=33/64, list 3
# longer than the 64 slots (evictions after they fill), the rest share the
# remainder
SIZES = [0, 1, 20, 200]


@pytest.fixture(scope="module")
def ext():
    from spark_rapids_ml_amd.ops.dispatch import hip_ops

    return hip_ops()


def _labels():
    rest = N - sum(SIZES)
    sizes = SIZES + [rest // 3, rest // 3, rest - 2 * (rest // 3)]
    lab = torch.repeat_interleave(torch.arange(NLIST), torch.tensor(sizes))
    g = torch.Generator().manual_seed(5)
    return lab[torch.randperm(N, generator=g)], sizes


_CASES = {}


def _case(d):
    """Items, labels and list centres for one d, built once with torch."""
    if d not in _CASES:
        g = torch.Generator().manual_seed(d)
        lab, sizes = _labels()
        centres = 3.0 * torch.randn(NLIST, d, generator=g)
        X = centres[lab] + torch.randn(N, d, generator=g)
        # one query next to each of five lists: with nprobe=1 they scan the
        # empty list, the single-row list, the short list and two long ones
        Q = centres[[2, 0, 1, 3, 5]] + 0.1 * torch.randn(5, d, generator=g)
        _CASES[d] = (X.cuda(), lab.cuda(), centres.cuda(), Q.cuda(), sizes)
    return _CASES[d]


def _true_keys(Q, X, ids, mode):
    x = X[ids.clamp(min=0)].double()
    q = Q[:, None, :].double()
    key = ((q - x) ** 2).sum(2) if mode == 0 else -(q * x).sum(2)
    return torch.where(ids >= 0, key, torch.full_like(key, float("inf")))


@pytest.mark.parametrize("k", [1, 33, 64])
@pytest.mark.parametrize("d", [1, 37, 64, 130])
def test_kernel_scan_matches_torch_scan(ext, d, k):
    X, lab, C, Q5, sizes = _case(d)
    for nq in (1, 5):
        Q = Q5[:nq].contiguous()
        for nprobe in (1, NLIST):
            for mode in (0, 1):
                key_t, ids_t = knn_mod._ivf_search(
                    Q, X, C, lab, NLIST, nprobe, k, mode, use_kernel=False
                )
                key_k, ids_k = knn_mod._ivf_search(
                    Q, X, C, lab, NLIST, nprobe, k, mode, use_kernel=True
                )
                tag = f"d={d} k={k} nq={nq} nprobe={nprobe} mode={mode}"
                assert key_k.shape == (nq, k) and ids_k.shape == (nq, k), tag
                # same number of filled slots; empty ones are (+inf, -1)
                assert torch.equal(ids_k < 0, ids_t < 0), tag
                assert torch.equal(torch.isinf(key_k), ids_k < 0), tag
                # where the indices differ (ties, rounding) the keys agree
                assert torch.allclose(key_k, key_t, rtol=1e-4, atol=1e-3), tag
                # the kernel's key is the key of the row it names
                true_k = _true_keys(Q, X, ids_k, mode)
                assert torch.allclose(key_k.double(), true_k, rtol=1e-4, atol=1e-3), tag
                # no row named twice
                for row in ids_k.cpu().numpy():
                    live = row[row >= 0]
                    assert len(set(live.tolist())) == len(live), tag
                # scanned lists are exactly the probed ones
                probe = knn_mod._probe_lists(Q, C, nprobe, mode)
                for qi in range(nq):
                    live = ids_k[qi][ids_k[qi] >= 0]
                    assert set(lab[live].tolist()) <= set(probe[qi].tolist()), tag
                    reachable = sum(sizes[l] for l in probe[qi].tolist())
                    assert live.numel() == min(k, reachable), tag


@pytest.mark.parametrize("k", [1, 33, 64])
def test_kernel_slots(ext, k):
    """Raw kernel output for one query against every list: live slots
    beyond a short list keep (+inf, -1), slots >= k are dead (-inf, -1)."""
    d = 37
    X, lab, C, Q5, sizes = _case(d)
    order = torch.argsort(lab)
    Xs = X[order].contiguous()
    off = torch.searchsorted(lab[order].contiguous(), torch.arange(NLIST + 1).cuda())
    lists = torch.arange(NLIST).cuda()
    zeros = torch.zeros(NLIST, dtype=torch.int64).cuda()
    for mode in (0, 1):
        key, pos = ext.ivf_scan_topk(
            Q5[:1].contiguous(), Xs, off, zeros, lists, lists.clone(), NLIST, k, mode
        )
        torch.cuda.synchronize()
        assert key.shape == (NLIST, 64) and pos.shape == (NLIST, 64)
        for l in range(NLIST):
            filled = min(k, sizes[l])
            p, kk = pos[l], key[l]
            assert int((p >= 0).sum()) == filled
            assert bool((p[k:] == -1).all()) and bool(torch.isneginf(kk[k:]).all())
            empty_live = (p[:k] < 0)
            assert int(empty_live.sum()) == k - filled
            assert bool(torch.isposinf(kk[:k][empty_live]).all())
            live = p[p >= 0]
            # positions stay inside the list's own row range
            assert bool(((live >= off[l]) & (live < off[l + 1])).all())
            # and are the list's best `filled` rows
            rows = Xs[off[l] : off[l + 1]].double()
            q = Q5[0].double()
            ref = ((q - rows) ** 2).sum(1) if mode == 0 else -(rows @ q)
            if filled:
                ref_best = torch.sort(ref).values[:filled]
                got = torch.sort(kk[p >= 0].double()).values
                assert torch.allclose(got, ref_best, rtol=1e-4, atol=1e-3)


def test_kernel_rejects_wide_rows(ext):
    Q = torch.zeros(1, 2049).cuda()
    X = torch.zeros(2, 2049).cuda()
    off = torch.tensor([0, 2]).cuda()
    z = torch.zeros(1, dtype=torch.int64).cuda()
    with pytest.raises(RuntimeError):
        ext.ivf_scan_topk(Q, X, off, z, z, z, 1, 1, 0)


def _count_kernel_calls(monkeypatch):
    calls = []
    real = knn_mod._ivf_scan_kernel

    def spy(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(knn_mod, "_ivf_scan_kernel", spy)
    return calls


@pytest.mark.parametrize("metric", NEW_METRICS)
def test_new_metrics_exact_at_full_probe_on_device(monkeypatch, metric):
    monkeypatch.delenv("SRML_IVF_KERNEL", raising=False)
    calls = _count_kernel_calls(monkeypatch)
    X = _data(500)
    Q = X[:50]
    idx, dist = _kneighbors(X, Q, 5, "ivfflat", {"nlist": 8, "nprobe": 8}, metric)
    assert calls, "the new metrics run the ivf_scan_topk kernel on the device"
    assert_exact(idx, dist, Q, X, metric, 5)


def test_euclidean_kernel_switch(monkeypatch):
    calls = _count_kernel_calls(monkeypatch)
    X = _data(500)
    # queries that are not items: the torch scan's q²+x²−2q·x expansion
    # cancels to ~1e-5 for a query equal to an item, which sqrt turns into
    # ~3e-3 — an error of that reference form, not of the kernel's
    # difference form (which gives exactly 0 there)
    Q = _data(50, seed=1)
    params = {"nlist": 8, "nprobe": 8}
    monkeypatch.setenv("SRML_IVF_KERNEL", "0")
    idx0, d0 = _kneighbors(X, Q, 5, "ivfflat", params, "euclidean")
    assert not calls
    monkeypatch.delenv("SRML_IVF_KERNEL")
    _kneighbors(X, Q, 5, "ivfflat", params, "euclidean")
    assert not calls, "euclidean keeps the torch scan by default"
    monkeypatch.setenv("SRML_IVF_KERNEL", "1")
    idx1, d1 = _kneighbors(X, Q, 5, "ivfflat", params, "euclidean")
    assert calls
    for a, b in zip(idx0, idx1):
        assert set(a.tolist()) == set(b.tolist())
    np.testing.assert_allclose(d1, d0, rtol=1e-4, atol=1e-3)
    assert_exact(idx1, d1, Q, X, "euclidean", 5)


@pytest.mark.parametrize("algorithm", ["brute", "rbc"])
def test_cosine_dbscan_on_device(algorithm):
    check_against_sklearn(cosine_fixture(), algorithm)
