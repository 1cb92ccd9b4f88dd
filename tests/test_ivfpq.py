"""IVF-PQ: n_bits, the index kept across kneighbors calls, and the torch ADC
scan against a numpy float64 ADC on an exact-integer synthetic index. The
synthetic index and the "valid top-k" assertions are shared with the GPU
test of the `ivfpq_scan_topk` kernel. Expected values never come from the
code under test."""

import numpy as np
import pytest
import torch

from spark_rapids_ml_amd import ApproximateNearestNeighbors
from spark_rapids_ml_amd.data import DataFrame
from spark_rapids_ml_amd.models import knn as knn_mod
from tests.test_ann_metrics import _data, _kneighbors, assert_exact

# -- synthetic exact-integer index -------------------------------------------
# empty, single row, shorter than a wave, 63/64/65 around one wave of rows,
# 257 = one block trip plus one row, 1100 = several trips with evictions
LIST_SIZES = [0, 1, 20, 63, 64, 65, 257, 1100]
NLIST = len(LIST_SIZES)
N_ITEMS = sum(LIST_SIZES)
NQ = 5
PQ_SHAPES = [(1, 1, 8), (3, 5, 8), (4, 4, 4), (75, 4, 8), (128, 1, 8)]  # (M, ds, n_bits)
K_CANDS = [1, 64, 65, 128, 256]
# nprobe=1: the short list, the empty one, the single row, the two long ones
PROBES = {
    1: np.array([[2], [0], [1], [6], [7]]),
    8: np.stack([np.roll(np.arange(NLIST), q) for q in range(NQ)]),
}

_SYNTH = {}


def synth_index(M, ds, n_bits):
    """Codebooks in [-3,3], Q and C in [-4,4], all integers: every LUT entry
    and every key is an integer below 2**24, exact in f32 in any summation
    order. Items are in a shuffled order; a few dozen rows of the two long
    lists are copies of other rows of the same list, so exact key ties
    exist. Returns numpy arrays."""
    key = (M, ds, n_bits)
    if key not in _SYNTH:
        rng = np.random.default_rng(1000 * M + 10 * ds + n_bits)
        d, ncodes = M * ds, 2**n_bits
        sorted_labels = np.repeat(np.arange(NLIST), LIST_SIZES)
        codes_s = rng.integers(0, ncodes, size=(N_ITEMS, M)).astype(np.uint8)
        for l in (6, 7):
            rows = np.flatnonzero(sorted_labels == l)
            picked = rng.choice(rows, size=40, replace=False)
            codes_s[picked[20:]] = codes_s[picked[:20]]
        perm = rng.permutation(N_ITEMS)  # item i is sorted row perm[i]
        _SYNTH[key] = {
            "codebooks": rng.integers(-3, 4, size=(M, ncodes, ds)).astype(np.float32),
            "C": rng.integers(-4, 5, size=(NLIST, d)).astype(np.float32),
            "Q": rng.integers(-4, 5, size=(NQ, d)).astype(np.float32),
            "labels": sorted_labels[perm],
            "codes": codes_s[perm],
        }
    return _SYNTH[key]


def adc_keys(ix, mode):
    """float64 ADC key of every (query, item): the item is its list centre
    plus its decoded residual. [NQ, N_ITEMS]."""
    cb = ix["codebooks"].astype(np.float64)
    M = cb.shape[0]
    codes = ix["codes"].astype(np.int64)
    recon = np.concatenate([cb[m][codes[:, m]] for m in range(M)], axis=1)
    approx = ix["C"].astype(np.float64)[ix["labels"]] + recon
    Q = ix["Q"].astype(np.float64)
    if mode == 1:
        return -(Q @ approx.T)
    return ((Q[:, None, :] - approx[None, :, :]) ** 2).sum(axis=2)


def assert_valid_topk(keys, ids, adc, labels, probe, k_cand, tag=""):
    """`keys`/`ids` [nq, k_cand] are a valid top-k_cand of the probed rows
    under `adc`, whichever way ties fell."""
    keys = np.asarray(keys, dtype=np.float64)
    ids = np.asarray(ids)
    assert keys.shape == (len(probe), k_cand) and ids.shape == keys.shape, tag
    for q in range(len(probe)):
        allowed = np.isin(labels, probe[q])
        want = np.sort(adc[q][allowed])[:k_cand]
        want = np.concatenate([want, np.full(k_cand - want.size, np.inf)])
        # the k_cand smallest keys over the probed rows, padded with +inf
        np.testing.assert_array_equal(np.sort(keys[q]), want, err_msg=f"{tag} q={q}")
        # -1 exactly where the key is +inf
        np.testing.assert_array_equal(ids[q] < 0, np.isinf(keys[q]), err_msg=f"{tag} q={q}")
        assert (ids[q][ids[q] < 0] == -1).all(), tag
        live = ids[q][ids[q] >= 0]
        # each id's own key is the key returned with it
        np.testing.assert_array_equal(adc[q][live], keys[q][ids[q] >= 0], err_msg=f"{tag} q={q}")
        assert len(set(live.tolist())) == live.size, f"{tag} q={q}: id named twice"
        assert allowed[live].all(), f"{tag} q={q}: id outside the probed lists"


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("M,ds,n_bits", PQ_SHAPES)
def test_torch_scan_matches_float64_adc(monkeypatch, M, ds, n_bits, mode):
    ix = synth_index(M, ds, n_bits)
    adc = adc_keys(ix, mode)
    assert np.abs(adc).max() < 2**24 and (adc == np.round(adc)).all()
    t = {name: torch.from_numpy(v) for name, v in ix.items()}
    for nprobe, probe in PROBES.items():
        # the scan picks its lists itself; pin them, integer centres tie
        monkeypatch.setattr(
            knn_mod, "_probe_lists", lambda *a, probe=probe: torch.from_numpy(probe)
        )
        for k_cand in (1, 65, 256):
            keys, ids = knn_mod._ivfpq_scan(
                t["Q"], t["C"], t["labels"], t["codebooks"], t["codes"],
                NLIST, nprobe, k_cand, mode,
            )
            assert_valid_topk(
                keys.numpy(), ids.numpy(), adc, ix["labels"], probe, k_cand,
                tag=f"nprobe={nprobe} k_cand={k_cand}",
            )


# -- n_bits ------------------------------------------------------------------
def test_n_bits_sets_the_codebook_size():
    Xt = torch.from_numpy(_data(600))
    index = knn_mod._ivfpq_build(Xt, {"nlist": 4, "M": 4, "n_bits": 4}, "euclidean")
    assert index.codebooks.shape == (4, 16, 4)
    assert int(index.codes.max()) < 16
    assert index.codes.dtype == torch.uint8 and index.codes.shape == (600, 4)
    assert index.n_bits == 4 and index.m_sub == 4
    # the list-sorted copy is the item-order codes, permuted
    assert torch.equal(index.codes_sorted[:, :4], index.codes[index.order])


def test_n_bits_defaults_to_eight():
    Xt = torch.from_numpy(_data(600))
    index = knn_mod._ivfpq_build(Xt, {"nlist": 4, "M": 4}, "euclidean")
    assert index.n_bits == 8 and index.codebooks.shape == (4, 256, 4)


@pytest.mark.parametrize("bad", [3, 9, "x"])
def test_n_bits_out_of_range_is_rejected(bad):
    Xt = torch.from_numpy(_data(600))
    with pytest.raises(ValueError, match="n_bits"):
        knn_mod._ivfpq_build(Xt, {"nlist": 4, "M": 4, "n_bits": bad}, "euclidean")
    model = ApproximateNearestNeighbors(
        k=3, algorithm="ivfpq", algoParams={"nlist": 4, "n_bits": bad}
    ).fit(DataFrame.from_numpy(_data(100)))
    with pytest.raises(ValueError, match="n_bits"):
        model.kneighbors(DataFrame.from_numpy(_data(5)))


@pytest.mark.parametrize("metric", ["euclidean", "inner_product"])
def test_four_bit_codes_are_exact_at_full_probe_and_full_refine(metric):
    X = _data(300)
    Q = X[:30]
    # k * refine_ratio = n: the refine re-ranks every item
    params = {"nlist": 8, "nprobe": 8, "n_bits": 4, "refine_ratio": 60.0}
    idx, dist = _kneighbors(X, Q, 5, "ivfpq", params, metric)
    assert_exact(idx, dist, Q, X, metric, 5)


# -- index cache ---------------------------------------------------------------
def _count_builds(monkeypatch):
    builds = []
    real = knn_mod._ivfpq_build

    def spy(*a, **kw):
        builds.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(knn_mod, "_ivfpq_build", spy)
    return builds


def _model(X, params, metric="euclidean"):
    return ApproximateNearestNeighbors(
        k=5, algorithm="ivfpq", algoParams=params, metric=metric
    ).fit(DataFrame.from_numpy(X))


def _query(model, Q):
    _, _, knn_df = model.kneighbors(DataFrame.from_numpy(Q))
    return np.asarray(knn_df["indices"]), np.asarray(knn_df["distances"])


def test_second_call_reuses_the_index(monkeypatch):
    monkeypatch.delenv("SRML_ANN_CACHE", raising=False)
    builds = _count_builds(monkeypatch)
    X = _data(500)
    model = _model(X, {"nlist": 8, "nprobe": 4})
    idx1, d1 = _query(model, X[:40])
    idx2, d2 = _query(model, X[:40])
    assert len(builds) == 1
    np.testing.assert_array_equal(idx1, idx2)
    np.testing.assert_array_equal(d1, d2)
    # other queries against the same index: still no build
    _query(model, X[40:60])
    assert len(builds) == 1


def test_changed_key_rebuilds(monkeypatch):
    monkeypatch.delenv("SRML_ANN_CACHE", raising=False)
    builds = _count_builds(monkeypatch)
    X = _data(500)
    model = _model(X, {"nlist": 8, "nprobe": 4})
    _query(model, X[:10])
    model._set_params(algoParams={"nlist": 8, "nprobe": 8})
    _query(model, X[:10])
    assert len(builds) == 2
    _query(model, X[:10])
    assert len(builds) == 2
    # a fresh model under another metric builds its own index
    other = _model(X, {"nlist": 8, "nprobe": 8}, metric="cosine")
    _query(other, X[:10])
    assert len(builds) == 3


def test_cache_can_be_switched_off(monkeypatch):
    monkeypatch.setenv("SRML_ANN_CACHE", "0")
    builds = _count_builds(monkeypatch)
    X = _data(500)
    model = _model(X, {"nlist": 8, "nprobe": 4})
    idx1, d1 = _query(model, X[:40])
    idx2, d2 = _query(model, X[:40])
    assert len(builds) == 2
    np.testing.assert_array_equal(idx1, idx2)
    np.testing.assert_array_equal(d1, d2)
