"""Prepared-X KMeans step (ops/kmeans.py `_prepared`, `_assign_prepared`).

The hi-plane split, the batched screen kernel and the inertia-fused
accumulation on exact (integer-valued) data, then the two-stage screen and
the cache through `kmeans_assign_reduce`, with a counting proxy around the
extension that shows which ops ran.
"""

import functools
import gc

import pytest
import torch

import spark_rapids_ml_amd.ops.kmeans as km

from .test_kmeans_split import make_case, ref_f64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ext():
    from spark_rapids_ml_amd.ops.dispatch import hip_ops

    return hip_ops()


@pytest.fixture(autouse=True)
def _empty_cache():
    km._drop_prepared()
    yield
    km._drop_prepared()


class Counting:
    """The extension; every op called through it is recorded by name, the
    split with its row count, the screen with its flagged count."""

    def __init__(self, real):
        self.real = real
        self.calls = []
        self.split_rows = []
        self.flagged = []

    def __getattr__(self, name):
        fn = getattr(self.real, name)

        def wrapped(*a, **kw):
            self.calls.append(name)
            out = fn(*a, **kw)
            if name == "kmeans_split_bf16":
                self.split_rows.append(a[0].shape[0])
            if name == "kmeans_argmin_kn_screen":
                self.flagged.append(int(out[4].item()))
            return out

        return wrapped


# ---------------------------------------------------------------------------
# 1. hi-plane split
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("m,d", [(257, 3000), (130, 37), (64, 8), (33, 1)])
def test_hi_split_equals_hi_half_of_full_split(ext, m, d):
    g = torch.Generator().manual_seed(3)
    A = (torch.randn(m, d, generator=g) * 3.0 + 1.5).cuda()
    mu = (torch.randn(d, generator=g) + 1.5).cuda()
    S, a_sq = ext.kmeans_split_bf16(A, mu)
    H, h_sq = ext.kmeans_split_bf16_hi(A, mu)
    dp = (d + 31) // 32 * 32
    assert H.shape == (m, dp) and H.dtype == torch.bfloat16 and H.is_contiguous()
    assert torch.equal(H.view(torch.int16), S[:, :dp].contiguous().view(torch.int16))
    assert torch.equal(h_sq.view(torch.int32), a_sq.view(torch.int32))
    assert not bool(H.view(torch.int16)[:, d:].any())


# ---------------------------------------------------------------------------
# 2. screen kernel on integer-valued blocks
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("k", [2, 7, 8, 9, 385, 1000])
@pytest.mark.parametrize("m", [1, 255, 257, 5000])
def test_screen_kernel_exact_on_integers(ext, m, k):
    """v = c_sq - 2 dot, a_sq (perfect squares) and the margins are small
    integers, so every comparison in the kernel and in the model is exact.
    Odd rows get a unique best planted; the others tie on their best, k being
    far larger than the range of v. Margin -1 leaves tied rows unflagged
    (a_sq >= 1), which shows the index a tie is given."""
    g = torch.Generator().manual_seed(100 * k + m)
    dots = torch.randint(-8, 9, (k, m), generator=g).float()
    c_sq = torch.randint(0, 8, (k,), generator=g).float()
    planted = torch.randint(0, k, (m,), generator=g)
    odd = torch.arange(m) % 2 == 1
    dots[planted[odd], torch.nonzero(odd).flatten()] = 100.0
    a_sq = (torch.randint(15, 19, (m,), generator=g) ** 2).float()
    a_sq[::7] = 1.0  # best + a_sq < 0 there: the clamp acts
    v = c_sq[:, None] - 2.0 * dots
    two = torch.topk(v, 2, dim=0, largest=False).values
    best, second = two[0], two[1]
    idx = torch.arange(k)[:, None].expand(k, m)
    lowest = torch.where(v == best[None, :], idx, torch.full_like(idx, k)).min(dim=0).values
    dd, aa, cc = dots.cuda(), a_sq.cuda(), c_sq.cuda()
    for ms in (0.0, 2.0, -1.0):
        flag = second <= best + ms * a_sq.sqrt()
        lb, md, it, flagged, nf = ext.kmeans_argmin_kn_screen(
            dd, aa, cc, torch.tensor([ms], device="cuda")
        )
        nf = int(nf.item())
        got = flagged[:nf].cpu().long().sort().values
        assert torch.equal(got, torch.nonzero(flag).flatten())
        if ms == 0.0:
            assert torch.equal(flag, second == best)  # only exact ties
        if ms == -1.0:
            assert not bool(flag.any())
        keep = ~flag
        d2 = (best + a_sq).clamp(min=0.0)
        assert torch.equal(lb.cpu().long()[keep], lowest[keep])
        assert torch.equal(md.cpu()[keep], d2[keep])
        assert float(it.item()) == float(d2[keep].double().sum())


# ---------------------------------------------------------------------------
# 3. accumulation with the inertia fused in
# ---------------------------------------------------------------------------

def _int_case(n, d, k, labels_from, seed):
    g = torch.Generator().manual_seed(seed)
    X = torch.randint(-3, 4, (n, d), generator=g).float()
    C = torch.randint(-2, 3, (k, d), generator=g).float()
    pool = torch.tensor(labels_from)
    labels = pool[torch.randint(0, pool.numel(), (n,), generator=g)].to(torch.int32)
    return X, C, labels


@pytest.mark.parametrize("vec", [True, False])
@pytest.mark.parametrize("n,d,k,labels_from", [
    (1000, 3000, 40, tuple(range(40))),
    (513, 4100, 3, (0, 1, 2)),      # d > 4096: the column loop runs twice
    (7, 5, 9, (0, 3, 8)),           # empty labels
    (257, 132, 4, (2,)),            # all rows in one label
    (1, 8, 2, (1,)),
])
def test_label_accumulate_inertia_exact(ext, n, d, k, labels_from, vec):
    """Small integers: every sum, f32 or f64, is exact, so sums and counts
    equal `label_accumulate` bit for bit and the inertia equals the f64
    reference."""
    X, C, labels = _int_case(n, d, k, labels_from, seed=n + d + k)
    Xg, Cg, lg = X.cuda(), C.cuda(), labels.cuda()
    sums, counts, inertia = ext.label_accumulate_inertia(Xg, lg, Cg, vec)
    ref_s, ref_c = ext.label_accumulate(Xg, lg, k)
    assert torch.equal(sums, ref_s) and torch.equal(counts, ref_c)
    host = torch.zeros(k, d, dtype=torch.float64).index_add_(0, labels.long(), X.double())
    assert torch.equal(sums.cpu().double(), host)
    assert torch.equal(counts.cpu().long(), torch.bincount(labels.long(), minlength=k))
    ref_in = float(((X.double() - C.double()[labels.long()]) ** 2).sum())
    assert inertia.dtype == torch.float64 and float(inertia.item()) == ref_in


# ---------------------------------------------------------------------------
# 4. two-stage screen through kmeans_assign_reduce
# ---------------------------------------------------------------------------

SHAPES = [(2049, 3000, 1000), (1025, 512, 384), (4096, 544, 385)]
N_PLANTED = 64
FAMILIES = ["blobs_0.05", "blobs_0.3", "blobs_0.05_shift", "blobs_0.3_shift", "ties", "randn"]


@functools.lru_cache(maxsize=None)
def make_family(name, n, d, k):
    """(X, C) on the CPU, built once per (family, shape) and never modified."""
    if name == "randn":
        return make_case("randn", n, d, k)
    g = torch.Generator().manual_seed(2024 + 7 * n + d + k)
    latent = torch.randn(k, d, generator=g)
    assign = torch.randint(0, k, (n,), generator=g)
    X = latent[assign] + 0.5 * torch.randn(n, d, generator=g)
    s = 0.3 if "0.3" in name else 0.05
    C = latent + s * torch.randn(k, d, generator=g)
    if name == "ties":
        # as tests/test_kmeans_split.py::make_case("ties"): x = (ca + cb)/2 +
        # delta (ca - cb) with delta |ca - cb|^2 = t |x||ca|, |t| = 2^-6 .. 2^-20
        e = torch.linspace(6.0, 20.0, N_PLANTED // 2)
        t = torch.cat([2.0 ** -e, -(2.0 ** -e)]).double()
        a = torch.arange(0, 2 * t.numel(), 2) % k
        ca, cb = C[a].double(), C[a + 1].double()
        mid = 0.5 * (ca + cb)
        D = ca - cb
        delta = t * mid.norm(dim=1) * ca.norm(dim=1) / (D * D).sum(1)
        X[torch.arange(t.numel()) * (n // t.numel())] = (mid + delta[:, None] * D).float()
    if name.endswith("shift"):
        X, C = X + 100.0, C + 100.0
    return X, C


def check_result(ext, X, C, labels, sums, counts, inertia):
    """The four properties every family must keep."""
    n, k = X.shape[0], C.shape[0]
    d2, ref_lab, gap = ref_f64(X, C)
    lab = labels.long()
    clear = gap > 1e-5 * X.double().norm(dim=1) * C.double().norm(dim=1)[ref_lab]
    assert torch.equal(lab[clear], ref_lab[clear])
    labels_p, _in_p = km._assign_gemm(ext, X, C, (X * X).sum(1), n, k, layout="kn")
    mism = labels != labels_p
    if bool(mism.any()):
        d_s = ((X[mism] - C[lab[mism]]) ** 2).sum(1)
        d_p = ((X[mism] - C[labels_p[mism].long()]) ** 2).sum(1)
        assert torch.allclose(d_s, d_p, rtol=1e-3, atol=1e-2)
    ref_in = float(d2.min(dim=1).values.clamp(min=0).sum())
    print(f"inertia {inertia!r} f64 {ref_in!r} rel {abs(inertia - ref_in) / max(1.0, ref_in):.3e}")
    assert abs(inertia - ref_in) <= 1e-4 * max(1.0, abs(ref_in))
    ref_s, ref_c = ext.label_accumulate(X, labels, k)
    assert torch.equal(counts, ref_c.double())
    # the split partials merge by atomics in either op: equal up to f32 order
    scale = float(ref_s.abs().max())
    assert torch.allclose(sums, ref_s.double(), rtol=1e-5, atol=1e-6 * max(1.0, scale))


@pytest.mark.parametrize("name", FAMILIES)
@pytest.mark.parametrize("n,d,k", SHAPES)
def test_two_stage_assign_reduce(ext, monkeypatch, n, d, k, name):
    Xh, Ch = make_family(name, n, d, k)
    X, C = Xh.cuda(), Ch.cuda()
    proxy = Counting(ext)
    monkeypatch.setattr(km, "hip_ops", lambda: proxy)
    monkeypatch.setattr(km, "F_HI", 0.25)
    monkeypatch.delenv("SRML_KMEANS_VARIANT", raising=False)
    monkeypatch.delenv("SRML_KMEANS_CACHE", raising=False)
    fell_back = []
    real_fb = km._fallback_f32
    monkeypatch.setattr(km, "_fallback_f32", lambda *a: fell_back.append(1) or real_fb(*a))

    labels, sums, counts, inertia = km.kmeans_assign_reduce(X, C, (X * X).sum(1))
    print(f"{name} {n}x{d} k={k}: ops {proxy.calls} flagged {proxy.flagged}")
    assert proxy.calls[0] == "kmeans_split_bf16_hi"
    assert "label_accumulate_inertia" in proxy.calls and not fell_back
    fell_up = n in proxy.split_rows  # the full split ran on X's rows
    if name == "randn":
        assert fell_up and proxy.calls.count("kmeans_argmin_kn_screen") == 2
    else:
        assert not fell_up and proxy.calls.count("kmeans_argmin_kn_screen") == 1
        assert proxy.flagged[0] <= 0.25 * n
    if name == "ties":
        assert proxy.flagged[0] > 0
    check_result(ext, X, C, labels, sums, counts, inertia)


@pytest.mark.parametrize("name", ["ties", "randn"])
def test_two_stage_chunked(ext, monkeypatch, name):
    """Row chunks of 600: every chunk is screened, and falls up, on its own."""
    n, d, k = SHAPES[0]
    Xh, Ch = make_family(name, n, d, k)
    X, C = Xh.cuda(), Ch.cuda()
    monkeypatch.setattr(km, "F_HI", 0.25)
    proxy = Counting(ext)
    x_sq = (X * X).sum(1)
    prep = km._prepared(proxy, X, C)
    labels, inertia = km._assign_prepared(
        proxy, X, C, x_sq, prep, max_dots_bytes=600 * k * 4
    )
    assert inertia is None
    chunks = -(-n // 600)
    stages = 2 if name == "randn" else 1
    assert proxy.calls.count("kmeans_argmin_kn_screen") == stages * chunks
    sums, counts, it = ext.label_accumulate_inertia(X, labels, C)
    check_result(ext, X, C, labels, sums.double(), counts.double(), float(it.item()))


# ---------------------------------------------------------------------------
# 5. the cache
# ---------------------------------------------------------------------------

def _blobs(n, d, k, seed):
    g = torch.Generator().manual_seed(seed)
    latent = torch.randn(k, d, generator=g)
    X = latent[torch.randint(0, k, (n,), generator=g)] + 0.5 * torch.randn(n, d, generator=g)
    C1 = latent + 0.05 * torch.randn(k, d, generator=g)
    C2 = latent + 0.3 * torch.randn(k, d, generator=g)
    return X.cuda(), C1.cuda(), C2.cuda()


def test_cache_reuse_rebuild_and_release(ext, monkeypatch):
    n, d, k = 1025, 512, 384
    X, C1, C2 = _blobs(n, d, k, seed=5)
    proxy = Counting(ext)
    monkeypatch.setattr(km, "hip_ops", lambda: proxy)
    monkeypatch.delenv("SRML_KMEANS_VARIANT", raising=False)
    monkeypatch.delenv("SRML_KMEANS_CACHE", raising=False)

    def step(X, C):
        proxy.calls.clear()
        proxy.split_rows.clear()
        out = km.kmeans_assign_reduce(X, C, (X * X).sum(1))
        check_result(ext, X, C, *out)
        return list(proxy.calls), list(proxy.split_rows)

    calls, _rows = step(X, C1)
    assert calls.count("kmeans_split_bf16_hi") == 1
    calls, rows = step(X, C2)  # same X, other centres: no split of X at all
    assert "kmeans_split_bf16_hi" not in calls and rows == [k]

    X.add_(1.0)  # bumps the version counter
    calls, _rows = step(X, C1 + 1.0)
    assert calls.count("kmeans_split_bf16_hi") == 1
    calls, _rows = step(X, C2 + 1.0)
    assert "kmeans_split_bf16_hi" not in calls

    Y = X.clone()  # another tensor of the same shape
    calls, _rows = step(Y, C1 + 1.0)
    assert calls.count("kmeans_split_bf16_hi") == 1
    assert km._PREP is not None and km._PREP.ref() is Y

    monkeypatch.setenv("SRML_KMEANS_CACHE", "0")
    calls, rows = step(Y, C1 + 1.0)
    # today's sequence: split C, split X, screen, [near-ties], label_accumulate
    assert calls[:3] == ["kmeans_split_bf16", "kmeans_split_bf16", "kmeans_argmin_kn_screen"]
    assert rows == [k, n] and calls[-1] == "label_accumulate"
    assert "kmeans_split_bf16_hi" not in calls and "label_accumulate_inertia" not in calls
    monkeypatch.delenv("SRML_KMEANS_CACHE")

    calls, _rows = step(Y, C2 + 1.0)  # the entry of Y outlived the switched-off call
    assert "kmeans_split_bf16_hi" not in calls
    del Y
    gc.collect()
    assert km._PREP is None


def test_cache_dropped_after_f32_fallback(ext, monkeypatch):
    """C = one row repeated: every row ties at both stages, the call ends in
    `_fallback_f32`, returns what the f32 path returns and leaves no entry."""
    n, d, k = 1025, 512, 384
    X, C1, _C2 = _blobs(n, d, k, seed=6)
    C = C1[:1].repeat(k, 1)
    proxy = Counting(ext)
    monkeypatch.setattr(km, "hip_ops", lambda: proxy)
    monkeypatch.delenv("SRML_KMEANS_VARIANT", raising=False)
    monkeypatch.delenv("SRML_KMEANS_CACHE", raising=False)
    fell_back = []
    real_fb = km._fallback_f32
    monkeypatch.setattr(km, "_fallback_f32", lambda *a: fell_back.append(1) or real_fb(*a))
    x_sq = (X * X).sum(1)
    km.kmeans_assign_reduce(X, C1, x_sq)
    assert km._PREP is not None
    labels, sums, counts, inertia = km.kmeans_assign_reduce(X, C, x_sq)
    assert fell_back == [1] and km._PREP is None
    assert proxy.calls[-1] == "label_accumulate"
    labels_p, inertia_p = km._assign_gemm(ext, X, C, x_sq, n, k, layout="kn")
    assert torch.equal(labels, labels_p)
    assert abs(inertia - float(inertia_p.item())) <= 1e-6 * float(inertia_p.item())
    calls_before = len(proxy.calls)
    km.kmeans_assign_reduce(X, C1, x_sq)  # re-centred on the next call
    assert proxy.calls[calls_before] == "kmeans_split_bf16_hi"
