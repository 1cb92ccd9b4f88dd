"""Random-forest ops: how one level's best splits are found and how rows are
rerouted, behind one small surface with two backends.

`forest_backend` picks the backend ONCE per grown forest from the device:

- HIP (gfx950): `rf_partition` (counting sort of rows by node) ->
  `rf_histogram` / `rf_histogram_fw` (LDS-privatized per-(node, feature
  chunk) histograms) -> `rf_best_split` (fused gain scan + argmax) ->
  `rf_reroute`.
- torch (CPU): `nonzero` / gather -> `index_add_` histograms ->
  `_best_split_class` / `_best_split_reg` -> gather reroute.

Both expose `partition(node_of_row, lut, B)`, `best_splits(feat_sel, mf, B,
min_leaf)` and `reroute(node_of_row, lut2, f, b, l, r)`; the grower in
`models/tree.py` drives them without knowing which one it holds. Forest
inference (`forest_predict`: `fil_predict` kernel or the level-wise torch
traversal) and the `SRML_RF_DEBUG` timer live here too.
"""

from __future__ import annotations

import os
import time
from typing import Callable, Dict, List, Optional

import numpy as np
import torch

from .dispatch import hip_ops, use_hip


class RFTimer:
    """SRML_RF_DEBUG=1: `[rf-debug]` lines and one `[rf-phase]` line per fit
    phase; =2: grow-loop time accumulated per label, `[rf-times]` at the end.
    Unset: every call is a no-op (no device sync)."""

    def __init__(self, device: torch.device):
        mode = os.environ.get("SRML_RF_DEBUG")
        self.verbose = mode == "1"
        self.accumulate = mode == "2"
        self.device = device
        self.acc: Dict[str, float] = {}
        self.t = time.perf_counter()

    def _now(self) -> float:
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        return time.perf_counter()

    def debug(self, msg: str) -> None:
        if self.verbose:
            print(f"[rf-debug] {msg}", flush=True)

    def phase(self, label: str) -> None:
        """Print the time since the previous phase (or construction)."""
        if self.verbose:
            t = self._now()
            print(f"[rf-phase] {label}: {t - self.t:.3f}s", flush=True)
            self.t = t

    def mark(self) -> None:
        if self.accumulate:
            self.t = self._now()

    def tick(self, label: str) -> None:
        """Add the time since the last mark/tick to `label`."""
        if self.accumulate:
            t = self._now()
            self.acc[label] = self.acc.get(label, 0.0) + (t - self.t)
            self.t = t

    def report(self) -> None:
        if self.accumulate:
            print(f"[rf-times] {sorted(self.acc.items(), key=lambda kv: -kv[1])}", flush=True)


# ---------------------------------------------------------------------------
# Split scan (torch)
# ---------------------------------------------------------------------------


def _max_lastdim(t: torch.Tensor):
    """(values, indices) over the last dim. torch-CPU's indexed max/argmax is
    ~30x slower than numpy in this build; route CPU through numpy."""
    if t.is_cuda:
        return t.max(dim=-1)
    arr = t.detach().numpy()
    idx = np.argmax(arr, axis=-1)
    vals = np.take_along_axis(arr, np.expand_dims(idx, -1), axis=-1).squeeze(-1)
    return torch.from_numpy(np.ascontiguousarray(vals)), torch.from_numpy(idx.astype(np.int64))


def _best_split_class(H: torch.Tensor, min_leaf: int):
    """H: [B,F,nb,C] class counts. Returns per (B,F): best gain (impurity
    decrease weighted by node fraction, Spark/CART gini), split bin, left/right
    class-count values, left count."""
    csum = H.cumsum(dim=2)  # left counts for split at bin b (bins <= b)
    total = csum[:, :, -1:, :]  # [B,F,1,C]
    left = csum[:, :, :-1, :]  # split bins 0..nb-2
    right = total - left
    lc = left.sum(dim=3)
    rc = right.sum(dim=3)
    nt = total.sum(dim=3)  # [B,F,1]
    gini = lambda cnt, tot: 1.0 - ((cnt / torch.clamp(tot.unsqueeze(-1), min=1e-12)) ** 2).sum(
        dim=-1
    )
    g_parent = gini(total, nt)  # [B,F,1]
    g_left = gini(left, lc)
    g_right = gini(right, rc)
    ntc = torch.clamp(nt, min=1e-12)
    gain = g_parent - (lc / ntc) * g_left - (rc / ntc) * g_right  # [B,F,nb-1]
    valid = (lc >= min_leaf) & (rc >= min_leaf)
    gain = torch.where(valid, gain, torch.full_like(gain, -1.0))
    best_gain, best_bin = _max_lastdim(gain)  # [B,F]
    B, F = best_gain.shape
    ar_b = torch.arange(B, device=H.device)[:, None].expand(B, F)
    ar_f = torch.arange(F, device=H.device)[None, :].expand(B, F)
    lval = left[ar_b, ar_f, best_bin]  # [B,F,C]
    rval = right[ar_b, ar_f, best_bin]
    lcnt = lc[ar_b, ar_f, best_bin]
    return best_gain, best_bin, lval, rval, lcnt


def _best_split_reg(H: torch.Tensor, min_leaf: int):
    """H: [B,F,nb,2] = (count,sum). Variance-reduction gain — the
    sum-of-squares terms cancel across parent/children, leaving
    (ls²/lc + rs²/rc - ts²/tc)/tc, so the histogram needs no y² channel."""
    cs = H.cumsum(dim=2)
    total = cs[:, :, -1:, :]
    left = cs[:, :, :-1, :]
    right = total - left
    lc, ls = left[..., 0], left[..., 1]
    rc, rs = right[..., 0], right[..., 1]
    tc, ts = total[..., 0], total[..., 1]
    lcc = torch.clamp(lc, min=1e-12)
    rcc = torch.clamp(rc, min=1e-12)
    tcc = torch.clamp(tc, min=1e-12)
    gain = (ls * ls / lcc + rs * rs / rcc - ts * ts / tcc) / tcc
    valid = (lc >= min_leaf) & (rc >= min_leaf)
    gain = torch.where(valid, gain, torch.full_like(gain, -1.0))
    best_gain, best_bin = _max_lastdim(gain)
    B, F = best_gain.shape
    ar_b = torch.arange(B, device=H.device)[:, None].expand(B, F)
    ar_f = torch.arange(F, device=H.device)[None, :].expand(B, F)
    lcb = lc[ar_b, ar_f, best_bin]
    lsb = ls[ar_b, ar_f, best_bin]
    rcb = rc[ar_b, ar_f, best_bin]
    rsb = rs[ar_b, ar_f, best_bin]
    lval = torch.stack([lsb / torch.clamp(lcb, min=1e-12), lcb], dim=-1)
    rval = torch.stack([rsb / torch.clamp(rcb, min=1e-12), rcb], dim=-1)
    return best_gain, best_bin, lval, rval, lcb


def _scan_chunk(H: torch.Tensor, classification: bool, min_leaf: int):
    """Torch twin of the rf_best_split kernel: per node the best (gain,
    column within the chunk, bin, left value, right value) of H [B,F,nb,C]."""
    scan = _best_split_class if classification else _best_split_reg
    gain, sbin, lval, rval, _ = scan(H, min_leaf)
    g, col = _max_lastdim(gain)
    ar = torch.arange(H.shape[0], device=H.device)
    return g, col, sbin[ar, col], lval[ar, col], rval[ar, col]


class _BestSplits:
    """Per-node running best over feature chunks. The merge is strict `>`,
    so the first chunk wins ties; a node no chunk could split keeps gain -1
    and feature -1."""

    def __init__(self, B: int, width: int, dev: torch.device):
        self.gain = torch.full((B,), -1.0, dtype=torch.float32, device=dev)
        self.feat = torch.full((B,), -1, dtype=torch.int64, device=dev)
        self.bin = torch.full((B,), -1, dtype=torch.int64, device=dev)
        self.lval = torch.zeros((B, width), dtype=torch.float32, device=dev)
        self.rval = torch.zeros((B, width), dtype=torch.float32, device=dev)

    def merge(self, g, feat, sbin, lval, rval) -> None:
        upd = g > self.gain
        self.gain = torch.where(upd, g, self.gain)
        self.feat = torch.where(upd, feat, self.feat)
        self.bin = torch.where(upd, sbin, self.bin)
        self.lval = torch.where(upd[:, None], lval, self.lval)
        self.rval = torch.where(upd[:, None], rval, self.rval)

    def result(self):
        return self.gain, self.feat, self.bin, self.lval, self.rval


# ---------------------------------------------------------------------------
# Level backends
# ---------------------------------------------------------------------------


class _TorchLevels:
    """Rows live in a VIRTUAL space [n_trees x per]; virtual row v maps to
    physical row sample[v] (bootstrap) or v % n."""

    label = "hip_hist=False"

    def __init__(self, Xb, y, task, n_classes, n_bins, sample, feat_chunk):
        self.Xb, self.n_bins, self.feat_chunk = Xb, n_bins, feat_chunk
        self.classification = task == "classification"
        self.width = n_classes if self.classification else 2
        self.y = y.to(torch.int64) if self.classification else y.to(torch.float32)
        self.phys = sample.to(torch.int64) if sample is not None else None

    def _physical(self, vrows: torch.Tensor) -> torch.Tensor:
        return self.phys[vrows] if self.phys is not None else vrows % self.Xb.shape[0]

    def partition(self, node_of_row, lut, B) -> bool:
        """Collect the batch's rows; False when no row is in the batch."""
        local = lut[node_of_row]
        rows = torch.nonzero(local >= 0).flatten()
        if rows.numel() == 0:
            return False
        self.loc = local[rows]
        self.prows = self._physical(rows)
        self.yb = self.y[self.prows]
        return True

    def _histogram(self, bins: torch.Tensor, B: int) -> torch.Tensor:
        """[B,F,nb,W] from bins [rows,F]: a row adds 1 to channel y
        (classification) or (1, y) to the two channels (regression: (count,
        sum) only — the sum-of-squares terms cancel in the gain)."""
        F, W, dev = bins.shape[1], self.width, bins.device
        col = torch.arange(F, device=dev)[None, :]
        cell = ((self.loc[:, None] * F + col) * self.n_bins + bins) * W
        hist = torch.zeros(B * F * self.n_bins * W, dtype=torch.float32, device=dev)
        ones = torch.ones(cell.numel(), device=dev)
        if self.classification:
            hist.index_add_(0, (cell + self.yb[:, None]).flatten(), ones)
        else:
            hist.index_add_(0, cell.flatten(), ones)
            hist.index_add_(0, (cell + 1).flatten(), self.yb[:, None].expand(-1, F).flatten())
        return hist.view(B, F, self.n_bins, W)

    def best_splits(self, feat_sel, mf, B, min_leaf):
        best = _BestSplits(B, self.width, self.Xb.device)
        ar = torch.arange(B, device=self.Xb.device)
        # sampled features: gather only the selected bytes of each row
        src = self.Xb[self.prows] if feat_sel is None else feat_sel[self.loc]
        for f0 in range(0, mf, self.feat_chunk):
            f1 = min(mf, f0 + self.feat_chunk)
            if feat_sel is None:
                bins = src[:, f0:f1].to(torch.int64)
            else:
                bins = self.Xb[self.prows[:, None], src[:, f0:f1]].to(torch.int64)
            g, col, sbin, lval, rval = _scan_chunk(
                self._histogram(bins, B), self.classification, min_leaf
            )
            feat = col + f0 if feat_sel is None else feat_sel[ar, col + f0]
            best.merge(g, feat, sbin, lval, rval)
        return best.result()

    def reroute(self, node_of_row, lut2, f, b, l, r) -> None:
        sl = lut2[node_of_row]
        mrows = torch.nonzero(sl >= 0).flatten()
        srel = sl[mrows]
        go_left = self.Xb[self._physical(mrows), f[srel]].to(torch.int64) <= b[srel]
        node_of_row[mrows] = torch.where(go_left, l[srel], r[srel])


class _HipLevels:
    """gfx950 kernels over node-sorted row segments. No call here syncs with
    the host except the one `y_max` read per forest."""

    label = "hip_hist=True"

    def __init__(self, ext, Xb, y, task, n_classes, n_bins, sample):
        self.ext, self.Xb, self.n_bins = ext, Xb, n_bins
        self.classification = task == "classification"
        self.n_classes = n_classes if self.classification else 0
        self.width = n_classes if self.classification else 2
        self.y32 = y.to(torch.int32) if self.classification else y.to(torch.float32)
        # max|y| for the packed regression histogram cells, ONE sync per fit
        self.y_max = 0.0
        if not self.classification:
            self.y_max = float(self.y32.abs().max().item()) if Xb.shape[0] else 0.0
            if self.y_max <= 0.0:
                self.y_max = 1.0
        self.sample = (
            sample.contiguous()
            if sample is not None
            else torch.empty(0, dtype=torch.int32, device=Xb.device)
        )
        # Measured dispatch (A/B in profiles/README.md): the row-lane kernel
        # wins for classification (sqrt-sampled features, sorted bootstrap =
        # dense segments), the feature-wide kernel wins for regression
        # (1/3-sampled features); SRML_RF_HIST=old|fw overrides
        mode = os.environ.get("SRML_RF_HIST")
        self.row_lane = mode == "old" or (mode != "fw" and self.classification)
        # features per launch: the node's histogram chunk fits 30 KB of LDS
        # (row-lane) or 150 KB (feature-wide)
        cells = max(1, n_bins * self.width)
        if self.row_lane:
            self.feat_chunk = max(1, min(512, (30 * 1024 // 4) // cells))
        else:
            self.feat_chunk = max(1, min(32, (150 * 1024 // 4) // cells))
        # column-major binned matrix for the row-lane histogram and reroute
        # kernels: a node segment's row gathers stay inside dense per-feature
        # cache lines (row-major fetched a ~47-line row to read ~54 sampled bytes)
        self.Xcm = Xb.T.contiguous()

    def partition(self, node_of_row, lut, B) -> bool:
        """Counting-sort partition kernel: one pass for counts, one scatter.
        Never reports an empty batch (that would be a host sync): it flows
        through as no-op kernels and an empty split set."""
        self.perm, self.seg_off = self.ext.rf_partition(node_of_row, lut, B)
        return True

    def best_splits(self, feat_sel, mf, B, min_leaf):
        dev = self.Xb.device
        if feat_sel is not None and not self.row_lane:
            # feature-wide kernel wants SORTED per-node subsets: a wave-load
            # then spans consecutive row bytes (avg gap d/mf), not the whole row
            feat_sel = feat_sel.sort(dim=1).values
        fsel32 = (
            feat_sel.to(torch.int32).contiguous()
            if feat_sel is not None
            else torch.empty((0, 0), dtype=torch.int32, device=dev)
        )
        hist_fn = self.ext.rf_histogram if self.row_lane else self.ext.rf_histogram_fw
        hist_x = self.Xcm if self.row_lane else self.Xb
        best = _BestSplits(B, self.width, dev)
        ar = torch.arange(B, device=dev)
        for f0 in range(0, mf, self.feat_chunk):
            F = min(mf, f0 + self.feat_chunk) - f0
            H = hist_fn(
                hist_x, self.perm, self.seg_off, fsel32, self.y32, f0, F,
                self.n_bins, self.n_classes, self.sample, self.y_max,
            )
            if H.shape[3] <= 16:
                # fused gain scan + per-node best (kernel)
                g, col, sbin, lval, rval = self.ext.rf_best_split(
                    H, min_leaf, self.classification
                )
                col = col.to(torch.int64) + f0
                # a node without a valid split reports column -1
                feat = col if feat_sel is None else feat_sel[ar, col.clamp(min=0)]
                sbin = sbin.to(torch.int64)
                if not self.classification:
                    lval, rval = self._mean_count(lval), self._mean_count(rval)
            else:
                # rf_best_split scans at most 16 channels: torch scan over
                # the kernel histogram past that
                g, col, sbin, lval, rval = _scan_chunk(H, self.classification, min_leaf)
                feat = col + f0 if feat_sel is None else feat_sel[ar, col + f0]
            best.merge(g, feat, sbin, lval, rval)
        return best.result()

    @staticmethod
    def _mean_count(v: torch.Tensor) -> torch.Tensor:
        """rf_best_split emits raw (count, sum); the tree stores (mean, count)."""
        return torch.stack([v[:, 1] / torch.clamp(v[:, 0], min=1e-12), v[:, 0]], dim=1)

    def reroute(self, node_of_row, lut2, f, b, l, r) -> None:
        """Single-pass kernel: gather split byte + child write fused."""
        self.ext.rf_reroute(
            node_of_row, lut2, f.to(torch.int32), b.to(torch.int32), l, r,
            self.Xcm, self.sample,
        )


def forest_backend(
    Xb: torch.Tensor,  # [n,d] uint8 binned
    y: torch.Tensor,  # [n] class idx (classification) or f32 target
    task: str,
    n_classes: int,
    n_bins: int,
    sample: Optional[torch.Tensor] = None,  # int32 virtual -> physical row map
    feat_chunk: int = 256,  # torch backend's features per histogram
):
    """The level backend for this forest, chosen once from the device."""
    if use_hip(Xb):
        return _HipLevels(hip_ops(), Xb, y, task, n_classes, n_bins, sample)
    return _TorchLevels(Xb, y, task, n_classes, n_bins, sample, feat_chunk)


# ---------------------------------------------------------------------------
# Inference
# ---------------------------------------------------------------------------


def forest_traverse(
    Xt: torch.Tensor, trees: List[Dict[str, np.ndarray]], task: str, n_classes: int
) -> torch.Tensor:
    """Vectorized level-wise torch traversal. Returns [n, C] vote sums
    (classification) or the [n] sum of tree means (regression)."""
    n, device = Xt.shape[0], Xt.device
    if task == "classification":
        acc = torch.zeros((n, n_classes), dtype=torch.float32, device=device)
    else:
        acc = torch.zeros(n, dtype=torch.float32, device=device)
    for t in trees:
        feature = torch.from_numpy(t["feature"]).to(device, torch.int64)
        thr = torch.from_numpy(t["threshold"]).to(device)
        left = torch.from_numpy(t["left"]).to(device, torch.int64)
        right = torch.from_numpy(t["right"]).to(device, torch.int64)
        leaf = torch.from_numpy(t["is_leaf"]).to(device)
        value = torch.from_numpy(t["value"]).to(device)
        node = torch.zeros(n, dtype=torch.int64, device=device)
        while True:
            at_leaf = leaf[node]
            if bool(at_leaf.all()):
                break
            f = feature[node].clamp(min=0)
            xv = Xt.gather(1, f.view(-1, 1)).flatten()
            # strict <: training partitions on bin(x) <= b  <=>  x <
            # edges[b] (=stored threshold), so rows equal to the
            # threshold went RIGHT during fit
            go_left = xv < thr[node]
            nxt = torch.where(go_left, left[node], right[node])
            node = torch.where(at_leaf, node, nxt)
        v = value[node]
        if task == "classification":
            acc += v / torch.clamp(v.sum(dim=1, keepdim=True), min=1e-12)
        else:
            acc += v[:, 0]
    return acc


def forest_predict(
    Xt: torch.Tensor,  # [n,d] f32
    trees: List[Dict[str, np.ndarray]],
    task: str,
    n_classes: int,
    arena: Callable[[torch.device], Dict[str, torch.Tensor]],
) -> torch.Tensor:
    """Forest inference, same return as `forest_traverse`. GPU: the
    fil_predict kernel — one thread walks every tree for its row over the
    flattened node arena `arena(device)` builds (the reference's FIL predict,
    tree.py:709-721); its per-thread vote registers hold up to 16 values.
    Otherwise the torch traversal."""
    width = n_classes if task == "classification" else 2
    if use_hip(Xt) and 0 < width <= 16 and Xt.shape[0] > 0 and len(trees) > 0:
        a = arena(Xt.device)
        out = hip_ops().fil_predict(
            Xt.contiguous(), a["feat"], a["thr"], a["left"], a["right"],
            a["value"], a["roots"], task == "classification",
        )
        return out if task == "classification" else out[:, 0]
    return forest_traverse(Xt, trees, task, n_classes)
