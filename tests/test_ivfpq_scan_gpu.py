"""GPU: the fused `ivfpq_scan_topk` kernel on the exact-integer synthetic
index of tests/test_ivfpq.py against a numpy float64 ADC, its host-side
argument checks, and IVF-PQ end to end on the device through the kernel."""

import numpy as np
import pytest
import torch

from spark_rapids_ml_amd.models import knn as knn_mod
from tests.test_ann_metrics import _data, _kneighbors, _recall, assert_exact, brute_force
from tests.test_ivfpq import (
    K_CANDS,
    LIST_SIZES,
    N_ITEMS,
    NLIST,
    NQ,
    PQ_SHAPES,
    PROBES,
    adc_keys,
    assert_valid_topk,
    synth_index,
)

pytestmark = pytest.mark.gpu

ALL_METRICS = ["euclidean", "l2", "sqeuclidean", "inner_product", "cosine"]


@pytest.fixture(scope="module")
def ext():
    from spark_rapids_ml_amd.ops.dispatch import hip_ops

    return hip_ops()


_DEV = {}


def _device_index(M, ds, n_bits):
    """The synthetic index on the device, list-sorted for the kernel."""
    key = (M, ds, n_bits)
    if key not in _DEV:
        ix = synth_index(M, ds, n_bits)
        order = np.argsort(ix["labels"], kind="stable")
        off = np.searchsorted(ix["labels"][order], np.arange(NLIST + 1))
        assert (np.diff(off) == LIST_SIZES).all()
        _DEV[key] = {
            "Q": torch.from_numpy(ix["Q"]).cuda(),
            "C": torch.from_numpy(ix["C"]).cuda(),
            "codebooks": torch.from_numpy(ix["codebooks"]).cuda(),
            "codes_s": torch.from_numpy(ix["codes"][order]).cuda().contiguous(),
            "list_off": torch.from_numpy(off).cuda(),
            "order": order,
        }
    return _DEV[key]


def _scan(ext, dev, probe, k_cand, mode):
    """One op call for every (query, probed list) pair, pairs sorted by list
    as the model path sorts them; then the per-query top-k_cand over the
    pairs' slots. Returns (raw keys, raw positions, keys, item ids)."""
    nq, nprobe = probe.shape
    flat = torch.from_numpy(probe.reshape(-1)).cuda()
    pair_out = torch.argsort(flat, stable=True)
    pair_list = flat[pair_out].contiguous()
    pair_q = torch.div(pair_out, nprobe, rounding_mode="floor")
    part_key, part_pos = ext.ivfpq_scan_topk(
        dev["Q"], dev["C"], dev["codebooks"], dev["codes_s"], dev["list_off"],
        pair_q, pair_list, pair_out, nq * nprobe, k_cand, mode,
    )
    torch.cuda.synchronize()
    raw_key, raw_pos = part_key.cpu().numpy(), part_pos.cpu().numpy()
    slots = raw_key.shape[1]
    pk = part_key.view(nq, nprobe * slots).masked_fill(
        part_pos.view(nq, nprobe * slots) < 0, float("inf")
    )
    vals, loc = torch.topk(pk, k_cand, dim=1, largest=False)
    pos = part_pos.view(nq, nprobe * slots).gather(1, loc).cpu().numpy()
    ids = np.where(pos >= 0, dev["order"][np.clip(pos, 0, None)], -1)
    return raw_key, raw_pos, vals.cpu().numpy(), ids


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("k_cand", K_CANDS)
@pytest.mark.parametrize("M,ds,n_bits", PQ_SHAPES)
def test_kernel_scan_is_a_valid_topk(ext, M, ds, n_bits, k_cand, mode):
    ix = synth_index(M, ds, n_bits)
    dev = _device_index(M, ds, n_bits)
    adc = adc_keys(ix, mode)
    off = dev["list_off"].cpu().numpy()
    for nprobe, probe in PROBES.items():
        tag = f"nprobe={nprobe}"
        raw_key, raw_pos, keys, ids = _scan(ext, dev, probe, k_cand, mode)
        slots = 64 if k_cand <= 64 else (128 if k_cand <= 128 else 256)
        assert raw_key.shape == (NQ * nprobe, slots) and raw_pos.shape == raw_key.shape, tag
        # slots >= k_cand are dead (-inf, -1); live empty ones (+inf, -1)
        assert np.isneginf(raw_key[:, k_cand:]).all() and (raw_pos[:, k_cand:] == -1).all(), tag
        live_key, live_pos = raw_key[:, :k_cand], raw_pos[:, :k_cand]
        np.testing.assert_array_equal(np.isposinf(live_key), live_pos < 0, err_msg=tag)
        assert (live_pos >= -1).all(), tag
        # each pair fills min(k_cand, list size) slots from its own list
        flat = probe.reshape(-1)
        for row, l in enumerate(flat):
            p = live_pos[row][live_pos[row] >= 0]
            assert p.size == min(k_cand, LIST_SIZES[l]), f"{tag} pair {row}"
            assert ((p >= off[l]) & (p < off[l + 1])).all(), f"{tag} pair {row}"
        assert_valid_topk(keys, ids, adc, ix["labels"], probe, k_cand, tag=tag)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("M,ds,n_bits", [(1, 1, 8), (3, 5, 8), (75, 4, 8)])
def test_model_path_scan_with_padded_code_rows(monkeypatch, M, ds, n_bits, mode):
    """`_ivfpq_scan_kernel` on an index whose list-sorted code rows are padded
    to a multiple of four bytes, as `_ivfpq_build` stores them: dword loads
    with a partly used last word. The pad bytes are 0xff, not zero, to show
    that they are never used as codes."""
    ix = synth_index(M, ds, n_bits)
    dev = _device_index(M, ds, n_bits)
    adc = adc_keys(ix, mode)
    padded = torch.full((N_ITEMS, (M + 3) // 4 * 4), 0xFF, dtype=torch.uint8).cuda()
    padded[:, :M] = dev["codes_s"]
    index = knn_mod.IvfPqIndex(
        Xt=dev["Q"], C=dev["C"], labels=torch.from_numpy(ix["labels"]).cuda(),
        order=torch.from_numpy(dev["order"]).cuda(), boundaries=dev["list_off"],
        codebooks=dev["codebooks"], codes=torch.from_numpy(ix["codes"]).cuda(),
        codes_sorted=padded, m_sub=M, n_bits=n_bits, mode=mode,
    )
    for nprobe, probe in PROBES.items():
        monkeypatch.setattr(
            knn_mod, "_probe_lists", lambda *a, probe=probe: torch.from_numpy(probe).cuda()
        )
        for k_cand in (64, 128):
            assert knn_mod._ivfpq_kernel_wanted(index, dev["Q"], k_cand)
            keys, ids = knn_mod._ivfpq_scan_kernel(index, dev["Q"], nprobe, k_cand)
            assert_valid_topk(
                keys.cpu().numpy(), ids.cpu().numpy(), adc, ix["labels"], probe, k_cand,
                tag=f"nprobe={nprobe} k_cand={k_cand}",
            )


# -- host-side argument checks -------------------------------------------------
def _args(M=4, ds=4, ncodes=16, d=None, n=8):
    d = M * ds if d is None else d
    z = torch.zeros(1, dtype=torch.int64).cuda()
    return [
        torch.zeros(1, d).cuda(),                            # Q
        torch.zeros(1, d).cuda(),                            # C
        torch.zeros(M, ncodes, ds).cuda(),                   # codebooks
        torch.zeros(n, M, dtype=torch.uint8).cuda(),         # codes_s
        torch.tensor([0, n]).cuda(),                         # list_off
        z, z.clone(), z.clone(),                             # pair_q, pair_list, pair_out
    ]


def test_wrapper_accepts_the_baseline_arguments(ext):
    key, pos = ext.ivfpq_scan_topk(*_args(), 1, 3, 0)
    torch.cuda.synchronize()
    # all-zero codes and codebooks: 8 rows of key 0, the best 3 kept
    assert key.shape == (1, 64) and (key[0, :3] == 0).all()
    assert sorted(pos[0, :3].tolist()) == sorted(set(pos[0, :3].tolist()))
    assert bool(((pos[0, :3] >= 0) & (pos[0, :3] < 8)).all())


def test_wrapper_rejects_bad_arguments(ext):
    a = _args()
    a[0] = a[0].double()
    with pytest.raises(RuntimeError):
        ext.ivfpq_scan_topk(*a, 1, 3, 0)  # Q not f32
    a = _args()
    a[3] = a[3].to(torch.int32)
    with pytest.raises(RuntimeError):
        ext.ivfpq_scan_topk(*a, 1, 3, 0)  # codes not u8
    with pytest.raises(RuntimeError):
        ext.ivfpq_scan_topk(*_args(d=17), 1, 3, 0)  # d != M * ds
    with pytest.raises(RuntimeError):
        ext.ivfpq_scan_topk(*_args(), 1, 0, 0)  # k_cand = 0
    with pytest.raises(RuntimeError):
        ext.ivfpq_scan_topk(*_args(), 1, 257, 0)  # k_cand = 257
    with pytest.raises(RuntimeError):
        ext.ivfpq_scan_topk(*_args(ncodes=48), 1, 3, 0)  # not a power of two
    with pytest.raises(RuntimeError, match="LDS"):
        ext.ivfpq_scan_topk(*_args(M=160, ds=1, ncodes=256), 1, 3, 0)  # 160 KB LUT
    a = _args()
    a[6] = torch.zeros(2, dtype=torch.int64).cuda()
    with pytest.raises(RuntimeError):
        ext.ivfpq_scan_topk(*a, 1, 3, 0)  # pair arrays differ in length


# -- model level ---------------------------------------------------------------
def _spy_on_op(monkeypatch, ext):
    calls = []
    real = ext.ivfpq_scan_topk

    def spy(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(ext, "ivfpq_scan_topk", spy)
    return calls


@pytest.mark.parametrize("metric", ALL_METRICS)
def test_ivfpq_exact_limit_runs_the_kernel(monkeypatch, ext, metric):
    monkeypatch.delenv("SRML_IVFPQ_KERNEL", raising=False)
    calls = _spy_on_op(monkeypatch, ext)
    X = _data(200, d=32)
    Q = _data(30, d=32, seed=1)
    # k_cand = k * refine_ratio = n = 200: the refine re-ranks every item
    params = {"nlist": 8, "nprobe": 8, "refine_ratio": 40}
    idx, dist = _kneighbors(X, Q, 5, "ivfpq", params, metric)
    assert calls, "ivfpq scans with the ivfpq_scan_topk kernel on the device"
    assert_exact(idx, dist, Q, X, metric, 5)


def test_kernel_switch_off_takes_the_torch_scan(monkeypatch, ext):
    calls = _spy_on_op(monkeypatch, ext)
    monkeypatch.setenv("SRML_IVFPQ_KERNEL", "0")
    X = _data(200, d=32)
    _kneighbors(X, X[:10], 5, "ivfpq", {"nlist": 8, "nprobe": 8}, "euclidean")
    assert not calls


@pytest.mark.parametrize("metric", ALL_METRICS)
def test_partial_probe_recall_kernel_against_torch(monkeypatch, ext, metric):
    """The two scans differ by f32 rounding of the ADC keys (difference form
    against expansion form), so only candidates at the k_cand boundary can
    swap: the kernel path's recall is at least the torch path's minus 0.01."""
    calls = _spy_on_op(monkeypatch, ext)
    X = _data(2000)
    Q = X[:100]
    params = {"nlist": 32, "nprobe": 8, "refine_ratio": 4}
    _, ref_i = brute_force(Q, X, metric, 10)
    monkeypatch.setenv("SRML_IVFPQ_KERNEL", "0")
    idx_t, _ = _kneighbors(X, Q, 10, "ivfpq", params, metric)
    assert not calls
    monkeypatch.setenv("SRML_IVFPQ_KERNEL", "1")
    idx_k, _ = _kneighbors(X, Q, 10, "ivfpq", params, metric)
    assert calls
    rec_t, rec_k = _recall(idx_t, ref_i), _recall(idx_k, ref_i)
    print(f"ivfpq {metric} recall@10: kernel {rec_k:.4f} torch {rec_t:.4f}")
    assert rec_k >= rec_t - 0.01, f"{metric}: kernel {rec_k} torch {rec_t}"
