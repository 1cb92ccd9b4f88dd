"""Row bounds of the KMeans step (ops/kmeans.py `_assign_bounded`).

The three kernels against torch models (`kmeans_bound_test` against the f64
inequality, with soundness against the brute-force argmin; `kmeans_centre_drift`
and the screen's gap output on integer-valued data, where every operation is
exact; `kmeans_gather_rows_bf16` bit for bit), then the driver: that a fit
takes the course it takes with SRML_KMEANS_BOUNDS=0, which steps are reference
passes, and what the kept state may alias or outlive.
"""

import functools

import pytest
import torch

import spark_rapids_ml_amd.ops.kmeans as km

from .test_kmeans_delta import _lloyd
from .test_kmeans_prepared import Counting, _blobs, check_result, make_family

pytestmark = pytest.mark.gpu

N, D, K = 1025, 512, 385


@pytest.fixture(scope="module")
def ext():
    from spark_rapids_ml_amd.ops.dispatch import hip_ops

    return hip_ops()


@pytest.fixture(autouse=True)
def _empty_cache(monkeypatch):
    for name in ("VARIANT", "CACHE", "DELTA", "BOUNDS"):
        monkeypatch.delenv("SRML_KMEANS_" + name, raising=False)
    km._drop_prepared()
    yield
    km._drop_prepared()


# ---------------------------------------------------------------------------
# 1. kmeans_bound_test against the f64 model of the inequality
# ---------------------------------------------------------------------------

def _scores(Xp, Cp):
    """v[i, j] = |c'_j|² − 2x'_i·c'_j in f64 from the f32-centred arrays."""
    Xd, Cd = Xp.double(), Cp.double()
    return (Cd * Cd).sum(1)[None, :] - 2.0 * Xd @ Cd.T


@functools.lru_cache(maxsize=None)
def bound_case(family):
    """Reference state and moved centres on the CPU, built once per family and
    never modified: (mu, Xp, C_ref, C_new, a_sq, lab_ref, gap_ref).

    gap_ref is the f64 (second − best) at C_ref rounded DOWN to f32, so it is
    a certified lower bound as the screen's is."""
    g = torch.Generator().manual_seed({"zero": 1, "small": 2, "far": 3, "dup": 4}[family])
    latent = torch.randn(K, D, generator=g)
    if family == "dup":  # centres 2i and 2i + 1 coincide (the last one stays single)
        latent[1::2] = latent[0:K - 1:2]
    X = latent[torch.randint(0, K, (N,), generator=g)] + 0.5 * torch.randn(N, D, generator=g)
    C_ref = latent.clone()
    mu = C_ref.mean(0)
    Xp, Cp = X - mu, C_ref - mu  # f32, as the split kernel centres
    v = _scores(Xp, Cp)
    if family == "dup":  # equal centres, equal scores, whatever order the GEMM summed in
        v[:, 1::2] = v[:, 0:K - 1:2]
    two, idx = torch.topk(v, 2, dim=1, largest=False)
    gap64 = two[:, 1] - two[:, 0]
    gap = gap64.float()
    gap = torch.where(gap.double() > gap64, torch.nextafter(gap, torch.zeros(())), gap)
    a_sq = (Xp.double() ** 2).sum(1).float()
    C_new = C_ref.clone()
    if family == "small":
        # scale chosen with `bound_model` below on the CPU: 76.3 % of the rows
        # pass and 7 lie within the slack (0.32 gives 98 %, 0.36 gives 24 %)
        C_new += 0.34 * torch.randn(K, D, generator=g)
    elif family == "far":
        C_new[7] += 5.0 * torch.randn(D, generator=g)
    elif family == "dup":
        C_new += 0.01 * torch.randn(K, D, generator=g)
    return mu, Xp, C_ref, C_new, a_sq, idx[:, 0].to(torch.int32), gap


def bound_model(mu, C_ref, C_new, a_sq, lab, gap):
    """(pass, |lhs − rhs|, slack) of the inequality of `kmeans_bound_test`, in f64."""
    cp, cr = (C_new - mu).double(), (C_ref - mu).double()
    Delta = (cp * cp).sum(1) - (cr * cr).sum(1)
    delta = (cp - cr).norm(dim=1)
    r = a_sq.double().sqrt()
    g = gap.double()
    a = lab.long()
    up = Delta[a] + 2.0 * r * delta[a]
    lo = Delta[None, :] - 2.0 * r[:, None] * delta[None, :]
    lo[torch.arange(lab.numel()), a] = float("inf")
    rhs = up - lo.min(dim=1).values
    slack = km.BOUND_SLACK * (Delta.abs().max() + 2.0 * r * delta.max()) + 2.0 ** -21 * g
    return (g > 0) & (g > rhs + slack), (g - rhs - slack).abs(), slack


@pytest.mark.parametrize("family", ["zero", "small", "far", "dup"])
def test_bound_test_against_f64_model(ext, family):
    mu, Xp, C_ref, C_new, a_sq, lab, gap = bound_case(family)
    passed, dist, slack = bound_model(mu, C_ref, C_new, a_sq, lab, gap)
    share = float(passed.float().mean())
    close = dist < slack
    print(f"{family}: model passes {100 * share:.1f} %, {int(close.sum())} rows within the slack")
    assert int(close.sum()) <= 0.01 * N  # the model alone stays within the 1 %
    if family == "zero":
        assert bool((gap > 0).all()) and bool(passed.all())
    if family == "small":
        assert 0.05 < share < 0.95
    if family == "far":
        assert 0.0 < share < 1.0
    if family == "dup":
        assert int((gap == 0).sum()) >= N - 8 and not bool(passed[gap == 0].any())

    Delta, delta = ext.kmeans_centre_drift(C_new.cuda(), C_ref.cuda(), mu.cuda())
    active, n_active = ext.kmeans_bound_test(
        gap.cuda(), lab.cuda(), a_sq.cuda(), Delta, delta, km.BOUND_SLACK
    )
    m = int(n_active.item())
    act = active[:m].cpu().long()
    assert act.unique().numel() == m and (m == 0 or (0 <= int(act.min()) and int(act.max()) < N))
    got = torch.ones(N, dtype=torch.bool)
    got[act] = False
    differ = got != passed
    assert bool(close[differ].all())
    assert not bool(got[gap == 0].any())  # strict: gap 0 never passes
    # soundness: a passed row keeps its label as the f64 argmin at the new centres
    new_lab = _scores(Xp, C_new - mu).argmin(dim=1)
    assert torch.equal(new_lab[got], lab.long()[got])


# ---------------------------------------------------------------------------
# 2. kmeans_centre_drift on integer-valued centres
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("d", [512, 515, 37])
def test_centre_drift_exact_on_integers(ext, d):
    g = torch.Generator().manual_seed(d)
    C = torch.randint(-8, 9, (K, d), generator=g).float()
    R = C + torch.randint(-3, 4, (K, d), generator=g).float()
    R[5] = C[5]  # one centre that did not move
    mu = torch.randint(-2, 3, (d,), generator=g).float()
    Delta, delta = ext.kmeans_centre_drift(C.cuda(), R.cuda(), mu.cuda())
    cp, cr = (C - mu).double(), (R - mu).double()
    assert torch.equal(Delta.cpu().double(), (cp * cp).sum(1) - (cr * cr).sum(1))
    want = ((cp - cr) ** 2).sum(1).sqrt()  # sqrt of an integer: correctly rounded
    up = want.float()
    up = torch.where(up.double() < want, torch.nextafter(up, torch.full((), float("inf"))), up)
    assert torch.equal(delta.cpu(), up)
    assert float(delta[5]) == 0.0 and float(Delta[5]) == 0.0


# ---------------------------------------------------------------------------
# 3. kmeans_gather_rows_bf16
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("m", [1, 63, 257])
def test_gather_rows_bit_equal(ext, m):
    n, dp = 1025, 512
    g = torch.Generator().manual_seed(m)
    H = torch.randn(n, dp, generator=g).to(torch.bfloat16).cuda()
    rows = torch.randint(0, n, (m + 5,), generator=g).to(torch.int32)
    rows[0] = n - 1
    out = ext.kmeans_gather_rows_bf16(H, rows.cuda(), m)
    assert out.shape == (m, dp) and out.dtype == torch.bfloat16 and out.is_contiguous()
    assert torch.equal(out.view(torch.int16), H[rows[:m].long().cuda()].view(torch.int16))


# ---------------------------------------------------------------------------
# 4. the screen's gap output
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("k", [9, 385])
@pytest.mark.parametrize("m", [255, 1025])
def test_screen_gap_output(ext, m, k):
    """Integer-valued block as in test_screen_kernel_exact_on_integers: v,
    sqrt(a_sq) and the margins are small integers, so second − best − margin
    is exact in the kernel and in the model."""
    g = torch.Generator().manual_seed(100 * k + m)
    dots = torch.randint(-8, 9, (k, m), generator=g).float()
    c_sq = torch.randint(0, 8, (k,), generator=g).float()
    planted = torch.randint(0, k, (m,), generator=g)
    odd = torch.arange(m) % 2 == 1
    dots[planted[odd], torch.nonzero(odd).flatten()] = 100.0
    a_sq = (torch.randint(15, 19, (m,), generator=g) ** 2).float()
    two = torch.topk(c_sq[:, None] - 2.0 * dots, 2, dim=0, largest=False).values
    best, second = two[0], two[1]
    dd, aa, cc = dots.cuda(), a_sq.cuda(), c_sq.cuda()
    for ms in (0.0, 2.0, -1.0):
        msd = torch.tensor([ms], device="cuda")
        flag = second <= best + ms * a_sq.sqrt()
        want = torch.where(flag, torch.zeros(m), second - best - ms * a_sq.sqrt())
        assert bool((want >= 0).all())
        gap = torch.full((m,), -7.0, device="cuda")
        new = ext.kmeans_argmin_kn_screen(dd, aa, cc, msd, gap_out=gap)
        old = ext.kmeans_argmin_kn_screen(dd, aa, cc, msd)
        assert len(new) == 5 and len(old) == 5
        assert torch.equal(gap.cpu(), want)
        keep = (~flag).cuda()  # labels and min_d of a flagged row are left to the refinement
        assert torch.equal(new[0][keep], old[0][keep]) and torch.equal(new[1][keep], old[1][keep])
        assert torch.equal(new[2], old[2]) and torch.equal(new[4], old[4])
        nf = int(new[4].item())
        assert nf == int(flag.sum())
        assert torch.equal(new[3][:nf].sort().values, old[3][:nf].sort().values)


# ---------------------------------------------------------------------------
# 5. the driver: a fit's course
# ---------------------------------------------------------------------------

class CountingBounds(Counting):
    """`Counting`, with the count `kmeans_bound_test` returned recorded too."""

    def __init__(self, real):
        super().__init__(real)
        self.active = []

    def __getattr__(self, name):
        fn = super().__getattr__(name)
        if name != "kmeans_bound_test":
            return fn

        def wrapped(*a, **kw):
            out = fn(*a, **kw)
            self.active.append(int(out[1].item()))
            return out

        return wrapped


def _took_bounds(calls):
    """The step's labels came from `_assign_bounded`: no screen over all rows."""
    return "kmeans_bound_test" in calls and (
        "kmeans_gather_rows_bf16" in calls or "kmeans_argmin_kn_screen" not in calls
    )


def test_fit_course_matches_unbounded_run(ext, monkeypatch):
    n, d, k = 2049, 512, 384
    X, _C1, C2 = _blobs(n, d, k, seed=7)
    proxy = CountingBounds(ext)
    monkeypatch.setattr(km, "hip_ops", lambda: proxy)
    shipped = _lloyd(ext, proxy, X, C2, steps=8)  # every step through check_result
    active = list(proxy.active)
    km._drop_prepared()
    monkeypatch.setenv("SRML_KMEANS_BOUNDS", "0")
    plain = _lloyd(ext, proxy, X, C2, steps=8)
    monkeypatch.delenv("SRML_KMEANS_BOUNDS")
    paths = ["bounds" if _took_bounds(s[3]) else "reference" for s in shipped]
    print("paths:", paths, "active:", active, "changed:", [s[5] for s in shipped])
    for a, b in zip(shipped, plain):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert "kmeans_bound_test" not in b[3] and "kmeans_centre_drift" not in b[3]
    assert "kmeans_bound_test" not in shipped[0][3]  # a fresh entry has no reference
    # the centres leave their start by more than the gaps allow, and how many
    # labels the first step changed is not known: a reference pass, untested
    assert "kmeans_bound_test" not in shipped[1][3] and paths[1] == "reference"
    assert len(active) == 6
    assert any(p == "bounds" and m < n for p, m in zip(paths[2:], active))


@pytest.mark.parametrize("variant", [None, "split_f64"])
def test_active_rows_take_the_screen(ext, monkeypatch, variant):
    """The planted near-ties of the "ties" family are flagged at the reference
    pass, keep gap 0 and stay active: the next step gathers them, screens them
    and decides them as the unbounded step does."""
    n, d, k = 1025, 512, 384
    Xh, Ch = make_family("ties", n, d, k)
    X, C = Xh.cuda(), Ch.cuda()
    if variant:
        monkeypatch.setenv("SRML_KMEANS_VARIANT", variant)
    proxy = CountingBounds(ext)
    monkeypatch.setattr(km, "hip_ops", lambda: proxy)
    g = torch.Generator().manual_seed(3)
    C2 = C + (1e-4 * torch.randn(k, d, generator=g)).cuda()
    x_sq = (X * X).sum(1)
    km.kmeans_assign_reduce(X, C, x_sq)
    km.kmeans_assign_reduce(X, C, x_sq)  # the labels stood still: the test is tried next
    near = int((km._PREP.gap_ref == 0).sum())
    proxy.calls.clear()
    out = km.kmeans_assign_reduce(X, C2, x_sq)
    calls = list(proxy.calls)
    print(f"near-ties {near}, active {proxy.active}, ops {calls}")
    assert _took_bounds(calls) and "kmeans_gather_rows_bf16" in calls
    assert 0 < near <= proxy.active[-1] < n
    assert ("kmeans_refine" in calls) == (variant == "split_f64")
    check_result(ext, X, C2, *out)
    km._drop_prepared()
    monkeypatch.setenv("SRML_KMEANS_BOUNDS", "0")
    plain = km.kmeans_assign_reduce(X, C2, x_sq)
    if variant == "split_f64":  # near-ties decided in f64: no rounding to differ by
        assert torch.equal(out[0], plain[0]) and torch.equal(out[2], plain[2])
    else:  # as check_result holds the screen to the f32 path
        mism = out[0] != plain[0]
        assert int(mism.sum()) <= near
        d_b = ((X[mism] - C2[out[0].long()[mism]]) ** 2).sum(1)
        d_p = ((X[mism] - C2[plain[0].long()[mism]]) ** 2).sum(1)
        assert torch.allclose(d_b, d_p, rtol=1e-3, atol=1e-2)


# ---------------------------------------------------------------------------
# 6. state hygiene
# ---------------------------------------------------------------------------

def test_state_hygiene(ext, monkeypatch):
    n, d, k = 1025, 512, 384
    X, C1, _C2 = _blobs(n, d, k, seed=5)
    proxy = CountingBounds(ext)
    monkeypatch.setattr(km, "hip_ops", lambda: proxy)
    g = torch.Generator().manual_seed(1)
    nudge = (1e-3 * torch.randn(k, d, generator=g)).cuda()

    def step(X, C):
        proxy.calls.clear()
        out = km.kmeans_assign_reduce(X, C, (X * X).sum(1))
        calls = list(proxy.calls)
        check_result(ext, X, C, *out)
        return out, calls

    out, calls = step(X, C1)
    assert "kmeans_bound_test" not in calls
    out, calls = step(X, C1)  # how many labels the first step changed is not known
    assert "kmeans_bound_test" not in calls and km._PREP.changed == 0
    state = km._PREP
    assert state.ref_k == k and torch.equal(state.C_ref, C1)
    assert out[0].data_ptr() != state.lab_ref.data_ptr()
    kept = state.lab_ref.clone()
    out[0].fill_(k - 1)  # the caller's labels are the caller's
    out, calls = step(X, C1 + nudge)
    assert _took_bounds(calls) and proxy.active[-1] < n
    assert torch.equal(state.lab_ref, kept) and torch.equal(state.C_ref, C1)
    assert out[0].data_ptr() != state.lab_ref.data_ptr()
    monkeypatch.setenv("SRML_KMEANS_BOUNDS", "0")
    ref, calls = step(X, C1 + nudge)
    assert "kmeans_bound_test" not in calls and torch.equal(ref[0], out[0])
    assert km._PREP.ref_k == 0  # a pass that stored no gaps leaves no reference
    monkeypatch.delenv("SRML_KMEANS_BOUNDS")
    _out, calls = step(X, C1)
    assert "kmeans_bound_test" not in calls and km._PREP.ref_k == k

    Ck = torch.cat([C1, C1[:16] + 1.0])  # another k on the same entry
    _out, calls = step(X, Ck)
    assert "kmeans_split_bf16_hi" not in calls and "kmeans_bound_test" not in calls
    assert km._PREP is state and state.ref_k == k + 16 and state.changed == n
    _out, calls = step(X, Ck)
    assert "kmeans_bound_test" not in calls
    _out, calls = step(X, Ck + torch.cat([nudge, nudge[:16]]))
    assert _took_bounds(calls)

    X.add_(1.0)  # a modified X: new entry, no reference
    _out, calls = step(X, Ck + 1.0)
    assert calls.count("kmeans_split_bf16_hi") == 1 and "kmeans_bound_test" not in calls
    assert km._PREP is not state

    monkeypatch.setenv("SRML_KMEANS_CACHE", "0")
    _out, calls = step(X, Ck + 1.0)
    assert "kmeans_bound_test" not in calls and "kmeans_centre_drift" not in calls
    monkeypatch.delenv("SRML_KMEANS_CACHE")


def test_chunked_reference_pass_stores_every_gap(ext):
    """Row chunks of 600: the gaps of both chunks reach the entry, and the
    bounded step after it agrees with the one after an unchunked pass. Two
    passes may differ in a dot by the f32 accumulation order of its d terms,
    d·2^-24·|x'||c'| at most, a gap holds four dots at weight 2."""
    n, d, k = 1025, 512, 384
    X, C1, _C2 = _blobs(n, d, k, seed=9)
    x_sq = (X * X).sum(1)
    g = torch.Generator().manual_seed(2)
    C = C1 + (1e-3 * torch.randn(k, d, generator=g)).cuda()
    runs = []
    for max_bytes in (8 << 30, 600 * k * 4):
        km._drop_prepared()
        proxy = CountingBounds(ext)
        prep = km._prepared(proxy, X, C1)
        first, _ = km._assign_prepared(proxy, X, C1, x_sq, prep, max_dots_bytes=max_bytes)
        assert proxy.calls.count("kmeans_argmin_kn_screen") == -(-n // min(n, max_bytes // (k * 4)))
        assert prep.ref_k == k and prep.gap_ref.shape == (n,)
        assert torch.equal(prep.lab_ref, first) and prep.lab_ref.data_ptr() != first.data_ptr()
        gap = prep.gap_ref.clone()
        proxy.calls.clear()
        labels, inertia = km._assign_prepared(proxy, X, C, x_sq, prep, max_dots_bytes=max_bytes)
        assert inertia is None and _took_bounds(proxy.calls) and proxy.active[-1] < n
        runs.append((gap, labels))
    (gap_a, lab_a), (gap_b, lab_b) = runs
    assert torch.equal(lab_a, lab_b)
    assert float((gap_b[600:] > 0).float().mean()) > 0.5  # the second chunk is there
    c_max = float((C1 - C1.mean(0)).norm(dim=1).max())
    tol = 8.0 * d * 2.0 ** -24 * km._PREP.a_sq.sqrt() * c_max
    assert bool(((gap_a - gap_b).abs() <= tol).all())
