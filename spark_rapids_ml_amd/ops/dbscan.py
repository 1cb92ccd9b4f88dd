"""DBSCAN ops: one clustering driver over two sweep backends.

`dbscan_backend` picks the backend ONCE per transform from the device:

- HIP (gfx950): the fused `dbscan_sweep` kernel keeps distances in registers
  and reduces into a 128-entry LDS accumulator. `algorithm="rbc"` (reference
  clustering.py:686-695) permutes rows by a coarse k-means partition so each
  128-row block / 128-column tile has a tight bounding ball, and every sweep
  walks only the column tiles admissible by the triangle inequality — same
  labels, a fraction of the O(N²) work when the data actually clusters.
- torch (CPU): row chunks of the [chunk, n] distance matrix, bounded by
  `max_mbytes_per_batch`.

Both expose `row0`, `n_rows` (this rank's slice in WORKING row order), `X`
(the working-order rows), `perm` (None, or int64 [n] with working row i ==
original row perm[i]), `neighbour_counts()` -> int32 [n_rows] (self
included) and `min_core_label(core_u8[n], labels_i32[n])` -> int32 [n_rows]
(INT32_MAX where a row has no core neighbour). `dbscan_labels` drives them
without knowing which one it holds. Exact: every sweep reduces over the FULL
eps-adjacency; no capped-graph approximation.
"""

from __future__ import annotations

import math
import os
import warnings

import numpy as np
import torch

from ..utils import as_numpy
from .dispatch import hip_ops, use_hip

INT32_MAX = torch.iinfo(torch.int32).max
MAX_SWEEPS = 64


def _debug() -> bool:
    return os.environ.get("SRML_DBSCAN_DEBUG") == "1"


def _coarse_assign(Xf, K: int, iters: int = 4, seed: int = 0, chunk_bytes: int = 1 << 30):
    """Coarse k-means partition used only to PERMUTE rows for ball-cover
    tile pruning (reference algorithm="rbc", clustering.py:686-695). The
    clustering result is exact regardless of this partition's quality — a
    bad partition only prunes fewer tiles."""
    n, d = Xf.shape
    ids = torch.randperm(n, generator=torch.Generator().manual_seed(seed))[:K]
    C = Xf[ids.to(Xf.device)].clone()
    x_sq = (Xf * Xf).sum(dim=1)
    asn = torch.empty(n, dtype=torch.int64, device=Xf.device)
    chunk = max(1, chunk_bytes // max(1, K * 4))
    for it in range(iters):
        c_sq = (C * C).sum(dim=1)
        for s in range(0, n, chunk):
            e = min(n, s + chunk)
            d2 = x_sq[s:e, None] + c_sq[None, :] - 2.0 * (Xf[s:e] @ C.T)
            asn[s:e] = d2.argmin(dim=1)
        if it + 1 < iters:
            sums = torch.zeros_like(C)
            cnts = torch.zeros(K, dtype=Xf.dtype, device=Xf.device)
            sums.index_add_(0, asn, Xf)
            cnts.index_add_(0, asn, torch.ones_like(x_sq))
            nz = cnts > 0
            C[nz] = sums[nz] / cnts[nz, None]
    return asn


def _tile_stats(Xp, B: int = 128):
    """Bounding ball (center, radius) of each consecutive B-row tile of Xp."""
    n, d = Xp.shape
    nfull = (n // B) * B
    cs, rs = [], []
    if nfull:
        Xv = Xp[:nfull].view(-1, B, d)
        c = Xv.mean(dim=1)
        r = (Xv - c[:, None, :]).pow(2).sum(dim=2).max(dim=1).values.sqrt()
        cs.append(c)
        rs.append(r)
    if n > nfull:
        c = Xp[nfull:].mean(dim=0, keepdim=True)
        r = (Xp[nfull:] - c).pow(2).sum(dim=1).max().sqrt().reshape(1)
        cs.append(c)
        rs.append(r)
    return torch.cat(cs, dim=0), torch.cat(rs, dim=0)


def _tile_lists(Xp, row0: int, n_rows: int, eps: float, B: int = 128,
                block_chunk: int = 8192):
    """CSR list of admissible 128-column tiles per 128-row block of the
    slice [row0, row0+n_rows): tile j can contain an eps-neighbor of a
    point in row block i only if ||c_i - c_j|| <= r_i + r_j + eps
    (triangle inequality — conservative, so the pruned sweep is exact).
    Returns (tile_idx int32, tile_off int32 [n_blocks+1], kept_fraction)."""
    cj, rj = _tile_stats(Xp, B)
    ci, ri = _tile_stats(Xp[row0:row0 + n_rows], B)
    nb, nt = ci.shape[0], cj.shape[0]
    cj_sq = (cj * cj).sum(dim=1)
    total = torch.zeros(1, dtype=torch.int64, device=Xp.device)
    offs = [total]
    idxs = []
    for s in range(0, nb, block_chunk):
        e = min(nb, s + block_chunk)
        d2 = ((ci[s:e] * ci[s:e]).sum(dim=1)[:, None] + cj_sq[None, :]
              - 2.0 * (ci[s:e] @ cj.T))
        thr = ri[s:e, None] + rj[None, :] + eps
        adm = d2 <= thr * thr * 1.0001 + 1e-5
        idxs.append(adm.nonzero()[:, 1].to(torch.int32))
        cum = adm.sum(dim=1).cumsum(0) + offs[-1][-1]
        offs.append(cum)
    tile_idx = torch.cat(idxs).contiguous()
    tile_off = torch.cat(offs).to(torch.int32).contiguous()
    kept = float(tile_idx.numel()) / float(max(1, nb * nt))
    return tile_idx, tile_off, kept


# ---------------------------------------------------------------------------
# Sweep backends
# ---------------------------------------------------------------------------


class _TorchSweeps:
    """Row chunks of the [chunk, n] squared-distance matrix. The masked label
    tensors are budgeted at 8 bytes per entry, so the chunk is bounded by
    bytes (reference max_mbytes_per_batch, clustering.py:673-682), defaulting
    to ~4 GB per intermediate. `algorithm` is ignored: every sweep is dense."""

    perm = None

    def __init__(self, Xf, off, n_local, eps2, max_mbytes_per_batch=None):
        self.X, self.row0, self.n_rows, self.eps2 = Xf, off, n_local, eps2
        n = Xf.shape[0]
        if max_mbytes_per_batch:
            self.chunk = max(1, int(max_mbytes_per_batch * 1e6 / (8 * max(1, n))))
        else:
            self.chunk = max(64, min(4096, (4 << 30) // (8 * max(1, n))))
        self.x_sq = (Xf * Xf).sum(dim=1)

    def _chunks(self):
        """(s, e, d2): squared distances of slice rows [s, e) to all rows."""
        X, x_sq = self.X, self.x_sq
        for s in range(0, self.n_rows, self.chunk):
            e = min(self.n_rows, s + self.chunk)
            rows = slice(self.row0 + s, self.row0 + e)
            yield s, e, x_sq[rows, None] + x_sq[None, :] - 2.0 * (X[rows] @ X.T)

    def neighbour_counts(self):
        counts = torch.empty(self.n_rows, dtype=torch.int32, device=self.X.device)
        for s, e, d2 in self._chunks():
            counts[s:e] = (d2 <= self.eps2).sum(dim=1)
        return counts

    def min_core_label(self, core_u8, labels):
        out = torch.empty(self.n_rows, dtype=torch.int32, device=self.X.device)
        is_core = core_u8.to(torch.bool)[None, :]
        big = labels.new_full((1,), INT32_MAX)
        for s, e, d2 in self._chunks():
            masked = torch.where(
                is_core & (d2 <= self.eps2), labels[None, :].expand(e - s, -1), big
            )
            out[s:e] = masked.min(dim=1).values
        return out


class _HipSweeps:
    """The fused `dbscan_sweep` kernel: mode 0 counts eps-neighbours, mode 1
    takes the minimum core-neighbour label; with `algorithm="rbc"` both walk
    the pruned tile lists of the permuted rows."""

    def __init__(self, ext, Xf, off, n_local, comm, eps2, algorithm):
        self.ext, self.eps2 = ext, eps2
        device = Xf.device
        n = Xf.shape[0]
        self.empty_u8 = torch.empty(0, dtype=torch.uint8, device=device)
        self.empty_i32 = torch.empty(0, dtype=torch.int32, device=device)
        self.perm = None
        self.tile_idx, self.tile_off = self.empty_i32, self.empty_i32
        self.row0, self.n_rows = off, n_local
        Xf = Xf.contiguous()
        if str(algorithm or "brute").lower() == "rbc" and n >= 4096:
            K = max(16, min(4096, n // 256))
            if comm.rank == 0:
                perm = torch.argsort(_coarse_assign(Xf, K), stable=True)
            else:
                perm = torch.empty(n, dtype=torch.int64, device=device)
            if comm.world_size > 1:
                perm = comm.broadcast(perm, src=0)
            self.perm = perm
            Xf = Xf[perm].contiguous()
            # balanced slice of the permuted rows
            base, rem = divmod(n, comm.world_size)
            self.n_rows = base + (1 if comm.rank < rem else 0)
            self.row0 = comm.rank * base + min(comm.rank, rem)
            tile_idx, tile_off, kept = _tile_lists(
                Xf, self.row0, self.n_rows, math.sqrt(eps2)
            )
            if _debug():
                print(f"[dbscan] rbc kept {kept:.3f} of column tiles", flush=True)
            if kept <= 0.95:
                self.tile_idx, self.tile_off = tile_idx, tile_off
            # else the ball bound prunes nothing (e.g. uniform noise): dense loop
        self.X = Xf
        self.x_sq = (Xf * Xf).sum(dim=1).contiguous()

    def _sweep(self, mode, core_u8, labels):
        return self.ext.dbscan_sweep(
            self.X, self.x_sq, self.row0, self.n_rows, self.eps2, mode,
            core_u8, labels, self.tile_idx, self.tile_off,
        )

    def neighbour_counts(self):
        return self._sweep(0, self.empty_u8, self.empty_i32)

    def min_core_label(self, core_u8, labels):
        return self._sweep(1, core_u8, labels.contiguous())


def dbscan_backend(Xf, off, n_local, comm, eps2, algorithm, max_mbytes_per_batch):
    """The sweep backend for this transform, chosen once from the device.
    Xf is the replicated [n, d] float32 dataset in original row order; this
    rank owns original rows [off, off + n_local)."""
    if use_hip(Xf):
        return _HipSweeps(hip_ops(), Xf, off, n_local, comm, eps2, algorithm)
    return _TorchSweeps(Xf, off, n_local, eps2, max_mbytes_per_batch)


# ---------------------------------------------------------------------------
# Driver
# ---------------------------------------------------------------------------


def dbscan_labels(backend, comm, off, n_local, min_samples) -> np.ndarray:
    """Cluster ids (int64 [n_local], -1 = noise, consecutive from 0 in order
    of each cluster's smallest working row) of original rows [off, off +
    n_local): core detection, min-label sweeps with pointer jumping to
    fixpoint over all-reduce(min), border assignment, relabel."""
    device = backend.X.device
    n = backend.X.shape[0]
    wo, wn = backend.row0, backend.n_rows
    BIG = INT32_MAX

    core_local = backend.neighbour_counts() >= min_samples
    core_full = torch.cat(
        comm.allgather_rows(core_local.to(torch.uint8)), dim=0
    ).to(torch.bool)
    if not bool(core_full.any()):
        # no core points anywhere -> every point is noise; the label sweeps
        # (2 more O(N^2) passes) are vacuous
        return np.full(n_local, -1, dtype=np.int64)
    core_u8 = core_full.to(torch.uint8).contiguous()

    labels = torch.arange(n, dtype=torch.int32, device=device)
    labels[~core_full] = BIG
    core_ids = torch.nonzero(core_full).flatten()

    def pointer_jump(lab):
        for _ in range(8):
            cur = lab[core_ids]
            tgt = lab[cur.long().clamp(max=n - 1)]
            tgt = torch.where(cur < BIG, tgt, cur)
            upd = torch.minimum(cur, tgt)
            if bool((upd == cur).all()):
                break
            lab[core_ids] = upd
        return lab

    for sweep in range(MAX_SWEEPS):
        out = backend.min_core_label(core_u8, labels)
        mine = labels[wo : wo + wn]
        new_full = torch.full((n,), BIG, dtype=torch.int32, device=device)
        new_full[wo : wo + wn] = torch.where(core_local, torch.minimum(mine, out), mine)
        new_full = comm.allreduce_t(new_full, "min")
        new_full[~core_full] = BIG
        new_full = pointer_jump(new_full)
        if bool((new_full == labels).all()):
            if _debug():
                print(f"[dbscan] converged after {sweep + 1} label sweeps", flush=True)
            break
        labels = new_full
    else:
        warnings.warn(
            f"DBSCAN label propagation did not converge in {MAX_SWEEPS} sweeps; "
            "clusters may be split",
            RuntimeWarning,
        )

    # border points: `out` was produced by the final (converged) sweep =
    # min core-neighbor label over the full adjacency; none -> noise
    final_work = torch.where(core_local, labels[wo : wo + wn], out).to(torch.int64)
    final_work[final_work == BIG] = -1

    full = np.concatenate(comm.allgather_obj(as_numpy(final_work)))  # working order
    if backend.perm is not None:
        orig = np.empty_like(full)
        orig[as_numpy(backend.perm)] = full
        full = orig
    # consecutive ids, ordered by each cluster's root row
    uniq = np.unique(full[full >= 0])
    v = full[off : off + n_local]
    return np.where(v >= 0, np.searchsorted(uniq, v), -1).astype(np.int64)
