"""GPU: the `cagra_prune` kernel on integer graphs against the numpy model of
tests/test_cagra_optimize.py (both outputs, array-equal), its host-side
argument checks, and the optimised cagra build on the device."""

import numpy as np
import pytest
import torch

from spark_rapids_ml_amd import ApproximateNearestNeighbors
from spark_rapids_ml_amd.data import DataFrame
from spark_rapids_ml_amd.models import knn as knn_mod
from tests.test_cagra_optimize import (
    OPT,
    any_ids,
    congruent_rows,
    distinct_rows,
    prune_cases,
    prune_model,
    prune_want,
)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ext():
    from spark_rapids_ml_amd.ops.dispatch import hip_ops

    return hip_ops()


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def _run(ext, G, d_out):
    P, detour = ext.cagra_prune(_i32(G), d_out)
    torch.cuda.synchronize()
    assert P.dtype == torch.int32 and detour.dtype == torch.int32
    assert tuple(P.shape) == (G.shape[0], d_out) and tuple(detour.shape) == G.shape
    return P.cpu().numpy().astype(np.int64), detour.cpu().numpy()


def _check(ext, G, d_out):
    want_P, want_detour = prune_model(G, d_out)
    P, detour = _run(ext, G, d_out)
    np.testing.assert_array_equal(detour, want_detour)
    np.testing.assert_array_equal(P, want_P)


@pytest.mark.parametrize("name", sorted(prune_cases()))
def test_kernel_equals_the_model_on_the_cpu_cases(ext, name):
    G, d_out, want_P, want_detour = prune_want(name)
    P, detour = _run(ext, G, d_out)
    np.testing.assert_array_equal(detour, want_detour)
    np.testing.assert_array_equal(P, want_P)


@pytest.mark.parametrize("D", [63, 64, 65])
def test_wave_boundary(ext, D):
    _check(ext, distinct_rows(300, D, seed=D), 32)
    _check(ext, any_ids(90, D, seed=100 + D), 32)  # repeats and self-loops


def test_widest_row(ext):
    _check(ext, distinct_rows(300, 256, seed=7), 128)
    _check(ext, any_ids(300, 256, seed=8), 128)
    _check(ext, distinct_rows(300, 256, seed=9), 256)  # D_out = D = 256 is accepted


def test_odd_sizes(ext):
    _check(ext, distinct_rows(200, 33, seed=10), 17)
    _check(ext, any_ids(150, 129, seed=11), 65)  # three row entries per lane
    _check(ext, distinct_rows(200, 192, seed=12), 192)


@pytest.mark.parametrize("modulus", [512, 64])
def test_ids_that_collide_in_a_table_indexed_by_low_bits(ext, modulus):
    """Every id of row u is congruent to u modulo 512, and modulo 64 = the
    2 * pow2ceil(32) slots the kernel's table has at D = 32."""
    G = congruent_rows(8192, 32, modulus, seed=modulus)
    assert ((G - np.arange(8192)[:, None]) % modulus == 0).all()
    _check(ext, G, 16)


def test_one_node(ext):
    P, detour = _run(ext, np.zeros((1, 1), dtype=np.int64), 1)
    np.testing.assert_array_equal(P, [[0]])
    np.testing.assert_array_equal(detour, [[-1]])


def test_more_nodes_than_blocks_in_flight(ext):
    _check(ext, distinct_rows(5000, 8, seed=13), 4)


# -- wrapper ----------------------------------------------------------------------
def test_wrapper_rejects_bad_arguments(ext):
    G = _i32(distinct_rows(64, 8, seed=0))
    ext.cagra_prune(G, 8)  # accepted, D_out = D
    with pytest.raises(RuntimeError, match="contiguous 2-d i32 device tensor"):
        ext.cagra_prune(G.long(), 4)  # i64
    with pytest.raises(RuntimeError, match="contiguous 2-d i32 device tensor"):
        ext.cagra_prune(G.cpu(), 4)  # host tensor
    with pytest.raises(RuntimeError, match="contiguous 2-d i32 device tensor"):
        ext.cagra_prune(G.t(), 4)  # not contiguous
    with pytest.raises(RuntimeError, match="contiguous 2-d i32 device tensor"):
        ext.cagra_prune(G.reshape(-1), 4)  # 1-d
    with pytest.raises(RuntimeError, match="D <= 256"):
        ext.cagra_prune(_i32(distinct_rows(300, 257, seed=1)), 4)  # D = 257
    ext.cagra_prune(_i32(distinct_rows(300, 256, seed=1)), 4)  # D = 256
    with pytest.raises(RuntimeError, match="D_out <= D"):
        ext.cagra_prune(G, 0)  # D_out = 0
    with pytest.raises(RuntimeError, match="D_out <= D"):
        ext.cagra_prune(G, 9)  # D_out > D
    P, detour = ext.cagra_prune(G[:0].contiguous(), 4)  # no nodes, no launch
    assert tuple(P.shape) == (0, 4) and tuple(detour.shape) == (0, 8)
    torch.cuda.synchronize()


# -- model level ------------------------------------------------------------------
def _spy(monkeypatch, ext, name, keep):
    calls = []
    real = getattr(ext, name)

    def spy(*a, **kw):
        calls.append(keep(a))
        return real(*a, **kw)

    monkeypatch.setattr(ext, name, spy)
    return calls


def test_optimised_build_runs_the_kernel_on_the_device(monkeypatch, ext):
    monkeypatch.delenv("SRML_CAGRA_KERNEL", raising=False)
    monkeypatch.delenv("SRML_CAGRA_PRUNE_KERNEL", raising=False)
    monkeypatch.delenv("SRML_ANN_CACHE", raising=False)
    prunes = _spy(monkeypatch, ext, "cagra_prune", lambda a: (tuple(a[0].shape), a[1]))
    searches = _spy(monkeypatch, ext, "cagra_search", lambda a: tuple(a[2].shape))
    X = np.random.default_rng(0).normal(size=(2000, 16)).astype(np.float32)
    model = ApproximateNearestNeighbors(k=10, algorithm="cagra", algoParams=dict(OPT)).fit(
        DataFrame.from_numpy(X)
    )
    q = DataFrame.from_numpy(X[:100])
    _, _, res = model.kneighbors(q)
    model.kneighbors(q)
    assert prunes == [((2000, 64), 32)], "one cagra_prune per build"
    assert searches == [(2000, 32), (2000, 32)]
    idx = np.asarray(res["indices"])
    assert ((idx >= 0) & (idx < 2000)).all()
    assert (idx[:, 0] == np.arange(100)).all()  # every query is an item


def test_torch_prune_on_the_device_gives_the_same_graph(monkeypatch, ext):
    monkeypatch.delenv("SRML_CAGRA_PRUNE_KERNEL", raising=False)
    prunes = _spy(monkeypatch, ext, "cagra_prune", lambda a: 1)
    X = np.random.default_rng(0).normal(size=(2000, 16)).astype(np.float32)
    G64 = knn_mod._cagra_knn_graph(torch.from_numpy(X).cuda(), 64, "nn_descent", 3)
    by_kernel = knn_mod._cagra_optimize(G64, 32)
    assert len(prunes) == 1
    monkeypatch.setenv("SRML_CAGRA_PRUNE_KERNEL", "0")
    by_torch = knn_mod._cagra_optimize(G64, 32)
    assert len(prunes) == 1
    assert by_kernel.dtype == torch.int32 and tuple(by_kernel.shape) == (2000, 32)
    np.testing.assert_array_equal(by_kernel.cpu().numpy(), by_torch.cpu().numpy())
