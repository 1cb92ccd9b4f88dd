"""k-NN: exact distributed brute force + approximate (IVF-Flat / IVF-PQ).

Exact (reference knn.py:76-835, NearestNeighborsMG): fit tags and stores the
item dataframe (reference knn.py:347-367); `kneighbors` computes, on every
rank, the top-k of ALL queries against the rank's LOCAL item shard (tiled
‖x−y‖² with the -2QIᵀ term on MFMA + per-tile top-k), then merges the
per-rank partial top-k. The reference moves partials with UCX p2p to
query-owner ranks (knn.py:763-774); here the partials ride one RCCL
all-gather over xGMI and every rank merges its own queries' candidates —
same O(P·q·k) traffic without a p2p mesh.

Approximate (reference knn.py:838-1723, cuVS): no comms — each rank builds a
local index over its item shard (IVF-Flat: k-means coarse quantizer reusing
the KMeans kernels; IVF-PQ: product quantization + exact refine), queries are
replicated, global top-k merged the same way as exact (reference does it via
Spark groupBy aggregation, knn.py:1282-1322). The `metric` param
(euclidean/l2/sqeuclidean/inner_product/cosine, reference knn.py:1007-1010)
is carried as a smaller-is-better key through search and merge — see the
convention table above `_ANN_METRICS`; on the GPU the IVF-Flat probed-list
scan is the fused `ivf_scan_topk` HIP kernel and the IVF-PQ ADC scan the
fused `ivfpq_scan_topk` kernel, and the cagra graph search the fused
`cagra_search` kernel. Every ANN index (IVF-Flat coarse lists, IVF-PQ, the
cagra graph) is built once per model and build-parameter set (`_cached_index`)
and queried by every later kneighbors call.
"""

from __future__ import annotations

import math
import os
import warnings
from dataclasses import dataclass
from typing import Any, Dict, Optional, Tuple

import numpy as np
import torch

from ..core import Estimator, Model, _FitContext
from ..data import DataFrame, extract_features, to_device_tensor
from ..params import (
    HasFeaturesCol,
    HasFeaturesCols,
    HasIDCol,
    Param,
    TypeConverters,
    DictTypeConverters,
)
from ..ops.knn import knn_topk
from ..utils import as_numpy


class _NNParams(HasFeaturesCol, HasFeaturesCols, HasIDCol):
    k = Param("knn", "k", "number of neighbors.", TypeConverters.toInt)

    def __init__(self, **kwargs: Any) -> None:
        super().__init__(**kwargs)
        self._setDefault(k=5)

    @classmethod
    def _param_mapping(cls) -> Dict[str, Optional[str]]:
        return {"k": "n_neighbors"}

    @classmethod
    def _get_native_params_default(cls) -> Dict[str, Any]:
        return {
            "n_neighbors": 5,
            "verbose": False,
            # cuML-signature knob accepted for ctor parity (inert here)
            "batch_size": 2000000,
        }

    def getK(self) -> int:
        return self.getOrDefault("k")

    # reference kNN exposes inputCol aliases over featuresCol (knn.py:203+)
    def setInputCol(self, value):
        if isinstance(value, (list, tuple)):
            return self._set_params(featuresCols=list(value))
        return self._set_params(featuresCol=value)

    def setInputCols(self, value):
        return self._set_params(featuresCols=list(value))

    def getInputCol(self):
        if self.isSet("featuresCols"):
            return self.getOrDefault("featuresCols")
        return self.getOrDefault("featuresCol")


class _NNModelBase(_NNParams, Model):
    """Shared kneighbors/join plumbing (reference _NNModelBase, knn.py:203+)."""

    def __init__(self, item_df: Optional[DataFrame] = None, **kwargs: Any) -> None:
        super().__init__(**kwargs)
        self._item_df = item_df

    def write(self):
        # persistence explicitly unsupported, matching the reference
        # (knn.py:384-408,484-508): the model is the raw item dataframe
        raise NotImplementedError(
            f"{type(self).__name__} does not support saving (reference parity)"
        )

    def save(self, path: str) -> None:
        self.write()

    def _transform_array(self, X: Any):  # pragma: no cover
        raise NotImplementedError("use kneighbors()/approxSimilarityJoin()")

    def transform(self, df: DataFrame) -> DataFrame:  # pragma: no cover
        raise NotImplementedError(
            "NearestNeighbors does not support transform(); use kneighbors()"
        )

    def _item_xy(self) -> Tuple[np.ndarray, np.ndarray]:
        features_col, features_cols = self._get_input_columns()
        X = extract_features(
            self._item_df, features_col, features_cols, self._float32_inputs
        )
        ids = np.asarray(self._item_df[self.getIdCol()])
        return X, ids

    def _query_xy(self, query_df: DataFrame) -> Tuple[np.ndarray, np.ndarray, DataFrame]:
        query_df = self._ensureIdCol(query_df)
        features_col, features_cols = self._get_input_columns()
        Q = extract_features(query_df, features_col, features_cols, self._float32_inputs)
        qids = np.asarray(query_df[self.getIdCol()])
        return Q, qids, query_df

    def _merge_partials(
        self,
        comm,
        my_dists: np.ndarray,  # [nq_total, k'] this rank's partial (k' <= k)
        my_ids: np.ndarray,
        nq_local: int,
        q_offset: int,
        k: int,
    ) -> Tuple[np.ndarray, np.ndarray]:
        """All-gather per-rank partial top-k (one fused tensor collective —
        the reference moves these with UCX p2p, knn.py:763-774) and merge
        for the local queries. Item ids ride as int32 bit-cast into the
        float buffer (one collective instead of a pickled-object gather).

        `my_dists` holds KEYS, smaller is better (for exact kNN the
        Euclidean distance is its own key); the caller converts the merged
        keys to the reported distance."""
        import torch as _torch

        kp = my_dists.shape[1]
        buf = np.concatenate(
            [
                np.ascontiguousarray(my_dists, dtype=np.float32),
                my_ids.astype(np.int32).view(np.float32),
            ],
            axis=1,
        )
        parts = comm.allgather_rows(_torch.from_numpy(buf))
        d_cat = np.concatenate([as_numpy(p)[:, :kp] for p in parts], axis=1)
        i_cat = np.concatenate(
            [
                np.ascontiguousarray(as_numpy(p)[:, kp:]).view(np.int32).astype(np.int64)
                for p in parts
            ],
            axis=1,
        )
        dl = d_cat[q_offset : q_offset + nq_local]
        il = i_cat[q_offset : q_offset + nq_local]
        order = np.argsort(dl, axis=1, kind="stable")[:, :k]
        rows = np.arange(dl.shape[0])[:, None]
        return dl[rows, order], il[rows, order]

    def _kneighbors_impl(
        self, query_df: DataFrame, search_fn, key_to_dist=None
    ) -> Tuple[DataFrame, DataFrame, DataFrame]:
        """`search_fn` returns (keys, idx) with smaller keys better and
        idx -1 for an empty slot; partials are padded with the worst key
        (+inf), merged on keys, and `key_to_dist` (None: the key is the
        distance, as for exact Euclidean kNN) maps the merged keys to the
        reported distances once, at the end."""
        from ..parallel.context import get_comm

        comm = get_comm()
        k = self.getK()
        X, item_ids = self._item_xy()
        Q, qids, query_df = self._query_xy(query_df)

        # replicate queries (reference broadcasts queries, knn.py:1250-1280)
        # — tensor all-gather over xGMI, not pickled objects
        import torch as _torch

        device = comm.device
        q_parts = comm.allgather_rows(
            to_device_tensor(np.ascontiguousarray(Q, dtype=np.float32), device)
        )
        Qt = _torch.cat(q_parts, dim=0)
        q_offset = sum(p.shape[0] for p in q_parts[: comm.rank])
        if X.shape[0] > 0:
            dists, idx = search_fn(Qt, X, k)
            idx_np = as_numpy(idx)
            ids_local = item_ids[idx_np]
            if (idx_np < 0).any():  # empty ANN slots keep id -1
                ids_local = np.where(idx_np >= 0, ids_local, -1)
            d_np = as_numpy(dists)
        else:
            d_np = np.full((Qt.shape[0], k), np.inf, dtype=np.float32)
            ids_local = np.full((Qt.shape[0], k), -1, dtype=np.int64)
        # pad to k columns for even merge
        if d_np.shape[1] < k:
            pad = k - d_np.shape[1]
            d_np = np.pad(d_np, ((0, 0), (0, pad)), constant_values=np.inf)
            ids_local = np.pad(ids_local, ((0, 0), (0, pad)), constant_values=-1)

        d_fin, i_fin = self._merge_partials(
            comm, d_np, ids_local, len(query_df), q_offset, k
        )
        if key_to_dist is not None:
            d_fin = key_to_dist(d_fin)
        knn_df = DataFrame(
            {
                f"query_{self.getIdCol()}": qids,
                "indices": i_fin,
                "distances": d_fin,
            }
        )
        return self._item_df, query_df, knn_df

    def exactNearestNeighborsJoin(
        self, query_df: DataFrame, distCol: str = "distCol"
    ) -> DataFrame:
        """Explode the kNN result into (item_id, query_id, distance) rows
        (reference knn.py:435-482)."""
        _, qdf, knn_df = self.kneighbors(query_df)
        qid = np.asarray(knn_df[f"query_{self.getIdCol()}"])
        idx = np.asarray(knn_df["indices"])
        dist = np.asarray(knn_df["distances"])
        k = idx.shape[1] if idx.ndim == 2 else 0
        return DataFrame(
            {
                f"query_{self.getIdCol()}": np.repeat(qid, k),
                f"item_{self.getIdCol()}": idx.reshape(-1),
                distCol: dist.reshape(-1),
            }
        )

    approxSimilarityJoin = exactNearestNeighborsJoin


class NearestNeighbors(_NNParams, Estimator):
    """Exact distributed brute-force kNN (reference NearestNeighbors,
    knn.py:203)."""

    def __init__(self, **kwargs: Any) -> None:
        super().__init__()
        self._set_params(**kwargs)

    def setK(self, value: int) -> "NearestNeighbors":
        return self._set_params(k=value)

    def setFeaturesCol(self, value) -> "NearestNeighbors":
        if isinstance(value, (list, tuple)):
            return self._set_params(featuresCols=list(value))
        return self._set_params(featuresCol=value)

    def fit(self, df: DataFrame, params=None) -> "NearestNeighborsModel":
        df = self._ensureIdCol(df)
        model = NearestNeighborsModel(item_df=df)
        self._copyValues(model)
        model._set_params(idCol=self.getIdCol())
        model._native_params = dict(self._native_params)
        model._float32_inputs = self._float32_inputs
        # MI355X-resident design: upload the item shard to HBM at fit time
        # (the reference's fit only tags rows, knn.py:347-367, and the first
        # search pays ingest; 288 GB/GPU lets the model live device-side)
        import torch as _torch

        if _torch.cuda.is_available():
            try:
                X, _ids = model._item_xy()
                if isinstance(X, np.ndarray):
                    from ..parallel.context import get_comm

                    Xt = to_device_tensor(
                        np.ascontiguousarray(X, dtype=np.float32), get_comm().device
                    )
                    model._item_dev = ((id(model._item_df), tuple(X.shape)), Xt)
            except Exception:
                pass
        return model

    def _fit_array(self, X, y, ctx, params):  # pragma: no cover
        raise NotImplementedError

    def _create_model(self, attrs):  # pragma: no cover
        raise NotImplementedError


class NearestNeighborsModel(_NNModelBase):
    """Exact kNN 'model' holding the item shard (reference
    NearestNeighborsModel, knn.py:511)."""

    def kneighbors(self, query_df: DataFrame) -> Tuple[DataFrame, DataFrame, DataFrame]:
        def search(Qt, X, k):
            from ..parallel.context import get_comm

            # cache the device-resident item shard across kneighbors calls
            # (re-uploading 30 GB of items dominated a 10M-item search);
            # keyed on the stored item_df + shape, which outlive the call
            key = (id(self._item_df), tuple(X.shape))
            cached = getattr(self, "_item_dev", None)
            if cached is None or cached[0] != key:
                Xt = to_device_tensor(
                    np.ascontiguousarray(X, dtype=np.float32), get_comm().device
                )
                self._item_dev = (key, Xt)
            else:
                Xt = cached[1]
            return knn_topk(Qt, Xt, k)

        return self._kneighbors_impl(query_df, search)


# ---------------------------------------------------------------------------
# Approximate kNN
# ---------------------------------------------------------------------------

# Metric convention. Every search function and the partial merge work on a
# KEY for which smaller is better; the key becomes the reported distance
# once, after the merge:
#
#   metric          preprocessing        key                 reported
#   euclidean, l2   -                    squared L2          sqrt(key)
#   sqeuclidean     -                    squared L2          key
#   cosine          unit-normalise rows  squared L2 of unit  key / 2  (= 1 - cos)
#   inner_product   -                    -q.x                -key, descending
#
# Rows are normalised by max(||.||, 1e-30), so a zero vector stays zero and
# comes out at cosine distance 0.5 from everything. An empty slot (fewer than
# k items reachable) has key +inf and id -1: it reports +inf for the ascending
# metrics and -inf for inner_product.
_ANN_METRICS = ("euclidean", "l2", "sqeuclidean", "inner_product", "cosine")
_MODE_L2, _MODE_DOT = 0, 1


def _check_metric(value: Any) -> str:
    if value not in _ANN_METRICS:
        raise ValueError(
            f"unsupported metric {value!r}; expected one of {', '.join(_ANN_METRICS)}"
        )
    return value


def _metric_mode(metric: str) -> int:
    return _MODE_DOT if metric == "inner_product" else _MODE_L2


def _normalize_rows(T: torch.Tensor) -> torch.Tensor:
    return T / T.norm(dim=1, keepdim=True).clamp_min(1e-30)


def _key_to_dist(key: np.ndarray, metric: str) -> np.ndarray:
    if metric == "inner_product":
        return -key
    key = np.maximum(key, 0.0)
    if metric == "sqeuclidean":
        return key
    if metric == "cosine":
        return key * np.float32(0.5)
    return np.sqrt(key)



class _ANNParams(_NNParams):
    algorithm = Param(
        "ann",
        "algorithm",
        "ivfflat|ivfpq|cagra (reference knn.py:1485-1524). cagra algoParams: "
        "graph_degree, nn_descent_niter, intermediate_graph_degree, "
        "build_algo (build); itopk_size, search_width, "
        "max_iterations (search).",
        TypeConverters.toString,
    )
    algoParams = Param(
        "ann", "algoParams", "algorithm tuning dict.", DictTypeConverters._toDict
    )

    metric = Param(
        "ann",
        "metric",
        "distance metric: euclidean|l2|sqeuclidean|inner_product|cosine "
        "(reference knn.py:1007-1010). ivfflat and ivfpq support all five; "
        "cagra supports euclidean|l2|sqeuclidean and raises for the other "
        "two. inner_product reports the raw dot products, largest first; "
        "cosine reports 1 - cos.",
        TypeConverters.toString,
    )

    def __init__(self, **kwargs: Any) -> None:
        super().__init__(**kwargs)
        self._setDefault(algorithm="ivfflat", algoParams=None, metric="euclidean")

    def setMetric(self, value: str):
        _check_metric(value)
        return self._set_params(metric=value)

    def getMetric(self) -> str:
        return self.getOrDefault("metric")


class ApproximateNearestNeighbors(_ANNParams, Estimator):
    """Approximate kNN (reference ApproximateNearestNeighbors, knn.py:935):
    per-rank local index, no fit-time comms."""

    def __init__(self, **kwargs: Any) -> None:
        super().__init__()
        self._set_params(**kwargs)

    def setK(self, value: int) -> "ApproximateNearestNeighbors":
        return self._set_params(k=value)

    def setAlgorithm(self, value: str) -> "ApproximateNearestNeighbors":
        return self._set_params(algorithm=value)

    def setAlgoParams(self, value: dict) -> "ApproximateNearestNeighbors":
        return self._set_params(algoParams=value)

    def setFeaturesCol(self, value) -> "ApproximateNearestNeighbors":
        if isinstance(value, (list, tuple)):
            return self._set_params(featuresCols=list(value))
        return self._set_params(featuresCol=value)

    def fit(self, df: DataFrame, params=None) -> "ApproximateNearestNeighborsModel":
        df = self._ensureIdCol(df)
        model = ApproximateNearestNeighborsModel(item_df=df)
        self._copyValues(model)
        model._set_params(idCol=self.getIdCol())
        model._native_params = dict(self._native_params)
        model._float32_inputs = self._float32_inputs
        return model

    def _fit_array(self, X, y, ctx, params):  # pragma: no cover
        raise NotImplementedError

    def _create_model(self, attrs):  # pragma: no cover
        raise NotImplementedError


class _ANNModelParams(_ANNParams):
    pass


class ApproximateNearestNeighborsModel(_ANNModelParams, _NNModelBase):
    """ANN model: local IVF index per rank (reference knn.py:1217)."""

    def approxSimilarityJoin(
        self, query_df: DataFrame, distCol: str = "distCol"
    ) -> DataFrame:
        """k-ANN join of query rows against the fitted items (reference
        approxSimilarityJoin, knn.py:1694-1723): exploded
        (item_id, query_id, distance) rows from this model's kneighbors."""
        return self.exactNearestNeighborsJoin(query_df, distCol=distCol)

    def _default_nlist(self, n: int) -> int:
        return _default_nlist(n)

    def _cached_index(self, algo: str, algo_params: Dict[str, Any], metric: str, build):
        """The index `build()` returns, kept across kneighbors calls under
        the key (algorithm, sorted algoParams items, metric); the item set is
        fixed per model, so nothing else can change it. One index is kept: a
        changed key rebuilds and replaces it. The cache is per rank (index
        builds run no collectives) and holds the index's device tensors for
        as long as the model lives. SRML_ANN_CACHE=0 builds on every call."""
        if os.environ.get("SRML_ANN_CACHE") == "0":
            return build()
        key = (
            algo,
            tuple(sorted((str(name), repr(v)) for name, v in algo_params.items())),
            metric,
        )
        kept = getattr(self, "_ann_index", None)
        if kept is None or kept[0] != key:
            kept = (key, build())
            self._ann_index = kept
        return kept[1]

    def kneighbors(self, query_df: DataFrame) -> Tuple[DataFrame, DataFrame, DataFrame]:
        algo = self.getOrDefault("algorithm").lower()
        algo_params = self.getOrDefault("algoParams") or {}
        # the constructor sets params without going through setMetric
        metric = _check_metric(self.getOrDefault("metric"))
        if algo in ("ivfflat", "ivf_flat"):
            search = self._make_ivfflat_search(algo_params, metric)
        elif algo in ("ivfpq", "ivf_pq"):
            search = self._make_ivfpq_search(algo_params, metric)
        elif algo == "cagra":
            if metric in ("cosine", "inner_product"):
                # the reference's cagra is sqeuclidean only (knn.py:1521-1524)
                raise ValueError(
                    f"cagra supports euclidean/l2/sqeuclidean, not {metric!r}"
                )
            search = self._make_cagra_search(algo_params, metric)
        else:
            raise ValueError(f"unsupported ANN algorithm {algo!r}")
        return self._kneighbors_impl(
            query_df, search, key_to_dist=lambda key: _key_to_dist(key, metric)
        )

    # -- CAGRA-equivalent graph ANN ---------------------------------------
    def _make_cagra_search(self, algo_params: Dict[str, Any], metric: str = "euclidean"):
        """Graph ANN (reference cuVS cagra, knn.py:1521-1524): nn-descent
        graph build, then a beam search that keeps itopk_size candidates and
        expands search_width of them per iteration. The graph
        (`_cagra_build`) is kept across calls by `_cached_index` under its
        build parameters alone, so the search parameters can change freely;
        each call runs `_cagra_query` on it. With `intermediate_graph_degree`
        or `build_algo` in algoParams the graph is cuVS's optimised one
        (`_cagra_optimize_params`), and the two resolved values join the key."""
        _cagra_search_params(algo_params, self.getK())  # fails before any work
        _cagra_optimize_params(algo_params, warn=False)  # as does a bad build parameter

        def search(Qt: torch.Tensor, X: np.ndarray, k: int):
            from ..parallel.context import get_comm

            device = get_comm().device

            def build():
                Xt = to_device_tensor(np.ascontiguousarray(X, dtype=np.float32), device)
                return _cagra_build(Xt, algo_params)

            build_params = {
                "graph_degree": int(algo_params.get("graph_degree", 32)),
                "nn_descent_niter": int(algo_params.get("nn_descent_niter", 3)),
            }
            optimize = _cagra_optimize_params(algo_params, X.shape[0], warn=False)
            if optimize is not None:
                build_params["intermediate_graph_degree"] = optimize[1]
                build_params["build_algo"] = optimize[2]
            index = self._cached_index("cagra", build_params, metric, build)
            itopk, width, max_it = _cagra_search_params(algo_params, k)
            return _cagra_query(index, Qt, k, itopk, width, max_it)

        return search

    # -- IVF-Flat ----------------------------------------------------------
    def _build_coarse(self, Xt: torch.Tensor, nlist: int, iters: int = 10):
        return _build_coarse(Xt, nlist, iters)

    def _make_ivfflat_search(self, algo_params: Dict[str, Any], metric: str = "euclidean"):
        def search(Qt: torch.Tensor, X: np.ndarray, k: int):
            from ..parallel.context import get_comm

            device = get_comm().device
            nlist = int(algo_params.get("nlist", self._default_nlist(X.shape[0])))
            nprobe = int(algo_params.get("nprobe", max(1, nlist // 16)))

            def build():
                Xt = to_device_tensor(np.ascontiguousarray(X, dtype=np.float32), device)
                if metric == "cosine":
                    Xt = _normalize_rows(Xt)
                return (Xt,) + tuple(self._build_coarse(Xt, nlist))

            # nprobe is a search parameter: only nlist shapes the index
            Xt, C, labels = self._cached_index("ivfflat", {"nlist": nlist}, metric, build)
            if metric == "cosine":
                Qt = _normalize_rows(Qt)
            mode = _metric_mode(metric)
            return _ivf_search(
                Qt, Xt, C, labels, nlist, nprobe, k, mode,
                use_kernel=_ivf_kernel_wanted(metric, Qt, Xt, k),
            )

        return search

    # -- IVF-PQ ------------------------------------------------------------
    def _make_ivfpq_search(self, algo_params: Dict[str, Any], metric: str = "euclidean"):
        """IVF-PQ with exact refine (reference ivf_pq + refine,
        knn.py:1512-1515,1643-1651): residual product quantization —
        per-subspace codebooks trained on coarse residuals,
        uint8 codes (2**n_bits codes per subspace), per-query ADC
        lookup-table candidate scan over the probed lists, then exact
        re-rank of refine_ratio*k candidates by the true metric. cosine runs
        the L2 pipeline on unit-normalised rows; inner_product scans with the
        dot-product ADC form. The index (`_ivfpq_build`) is kept across calls
        by `_cached_index`; each call runs `_ivfpq_query` on it."""
        _ivfpq_n_bits(algo_params)  # a bad n_bits fails before any work

        def search(Qt: torch.Tensor, X: np.ndarray, k: int):
            from ..parallel.context import get_comm

            device = get_comm().device

            def build():
                Xt = to_device_tensor(np.ascontiguousarray(X, dtype=np.float32), device)
                return _ivfpq_build(Xt, algo_params, metric)

            index = self._cached_index("ivfpq", algo_params, metric, build)
            if metric == "cosine":
                Qt = _normalize_rows(Qt)
            nlist = index.boundaries.numel() - 1
            nprobe = int(algo_params.get("nprobe", max(1, nlist // 16)))
            refine = float(algo_params.get("refine_ratio", 2.0))
            return _ivfpq_query(index, Qt, k, nprobe, refine)

        return search


def _default_nlist(n: int) -> int:
    return max(1, min(1024, int(math.sqrt(max(1, n)))))


def _build_coarse(Xt: torch.Tensor, nlist: int, iters: int = 10):
    """Local k-means coarse quantizer (reuses the KMeans assign kernel)."""
    from ..ops import kmeans_assign_reduce

    n = Xt.shape[0]
    g = torch.Generator(device="cpu")
    g.manual_seed(42)
    sel = torch.randperm(n, generator=g)[:nlist].to(Xt.device)
    C = Xt[sel].clone()
    x_sq = (Xt * Xt).sum(dim=1)
    for _ in range(iters):
        labels, sums, counts, _ = kmeans_assign_reduce(Xt, C, x_sq)
        ne = counts > 0
        C[ne] = (sums[ne] / counts[ne, None]).to(C.dtype)
    labels, _, _, _ = kmeans_assign_reduce(Xt, C, x_sq)
    return C, labels.to(torch.int64)


def _ivf_search(
    Qt: torch.Tensor,
    Xt: torch.Tensor,
    C: torch.Tensor,
    labels: torch.Tensor,
    nlist: int,
    nprobe: int,
    k: int,
    mode: int = _MODE_L2,
    use_kernel: bool = False,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Probe the nprobe best lists per query and keep a running top-k.
    Returns (keys [nq, k], item rows [nq, k]); the key is the squared L2
    distance (mode 0) or -q.x (mode 1), +inf with row -1 for an empty slot.
    `use_kernel` scans the probed lists with the fused `ivf_scan_topk` HIP
    kernel; otherwise a torch loop over the lists."""
    device = Qt.device
    nq = Qt.shape[0]
    nprobe = min(nprobe, nlist)
    probe = _probe_lists(Qt, C, nprobe, mode)  # [nq, nprobe]
    order = torch.argsort(labels)
    sorted_labels = labels[order]
    boundaries = torch.searchsorted(
        sorted_labels, torch.arange(nlist + 1, device=device)
    )
    if use_kernel:
        return _ivf_scan_kernel(Qt, Xt, order, boundaries, probe, k, mode)

    probe_mask = torch.zeros((nq, nlist), dtype=torch.bool, device=device)
    probe_mask.scatter_(1, probe, True)
    best_d = torch.full((nq, k), float("inf"), device=device)
    best_i = torch.full((nq, k), -1, dtype=torch.int64, device=device)
    for l in range(nlist):
        s, e = int(boundaries[l]), int(boundaries[l + 1])
        if s == e:
            continue
        qsel = torch.nonzero(probe_mask[:, l]).flatten()
        if qsel.numel() == 0:
            continue
        items = order[s:e]
        kb = min(k, e - s)
        qb = Qt[qsel]
        xb = Xt[items]
        if mode == _MODE_DOT:
            d2 = -(qb @ xb.T)
        else:
            d2 = (
                (qb * qb).sum(dim=1)[:, None]
                + (xb * xb).sum(dim=1)[None, :]
                - 2.0 * (qb @ xb.T)
            )
        vals, loc = torch.topk(d2, kb, dim=1, largest=False)
        ids = items[loc]
        # merge with running top-k
        cat_d = torch.cat([best_d[qsel], vals], dim=1)
        cat_i = torch.cat([best_i[qsel], ids], dim=1)
        mvals, morder = torch.topk(cat_d, k, dim=1, largest=False)
        rows = torch.arange(qsel.numel(), device=device)[:, None]
        best_d[qsel] = mvals
        best_i[qsel] = cat_i[rows, morder]
    return best_d, best_i


def _probe_lists(Qt: torch.Tensor, C: torch.Tensor, nprobe: int, mode: int) -> torch.Tensor:
    """The nprobe lists to scan per query: smallest L2 to the list centre,
    or largest q.c for the dot-product key."""
    if mode == _MODE_DOT:
        return (Qt @ C.T).topk(nprobe, dim=1, largest=True).indices
    cd = (
        (Qt * Qt).sum(dim=1)[:, None]
        + (C * C).sum(dim=1)[None, :]
        - 2.0 * (Qt @ C.T)
    )
    return cd.topk(nprobe, dim=1, largest=False).indices


def _ivf_kernel_wanted(metric: str, Qt: torch.Tensor, Xt: torch.Tensor, k: int) -> bool:
    """Route the IVF-Flat scan through the `ivf_scan_topk` kernel? On the GPU
    (f32, k <= 64, d <= 2048) the metrics this kernel introduced use it;
    euclidean/l2 keep the torch path unless SRML_IVF_KERNEL=1, and
    SRML_IVF_KERNEL=0 forces the torch path for every metric."""
    from ..ops.dispatch import use_hip

    env = os.environ.get("SRML_IVF_KERNEL")
    if env == "0" or not (Qt.is_cuda and use_hip(Qt, Xt)):
        return False
    if Qt.dtype != torch.float32 or Xt.dtype != torch.float32:
        return False
    if k > 64 or Qt.shape[1] > 2048:
        return False
    if metric in ("euclidean", "l2"):
        return env == "1"
    return True


def _ivf_scan_kernel(
    Qt: torch.Tensor,
    Xt: torch.Tensor,
    order: torch.Tensor,
    boundaries: torch.Tensor,
    probe: torch.Tensor,
    k: int,
    mode: int,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Kernel path of `_ivf_search`: one wave per (query, probed list) pair
    over the list-sorted item copy, 64 key/position slots per pair, then one
    topk over each query's nprobe*64 slots. The pairs are sorted by list so
    neighbouring waves stream the same rows through L2; each pair still
    writes its own [query, probe] output row."""
    from ..ops.dispatch import hip_ops

    ext = hip_ops()
    nq, nprobe = probe.shape
    Xs = Xt[order].contiguous()
    list_off = boundaries.to(torch.int64).contiguous()
    keys = torch.empty((nq, k), dtype=torch.float32, device=Qt.device)
    ids = torch.empty((nq, k), dtype=torch.int64, device=Qt.device)
    # key (f32) + position (i64) slot buffers stay under 512 MB per chunk
    qchunk = max(1, (512 << 20) // (nprobe * 64 * 12))
    for s in range(0, nq, qchunk):
        e = min(nq, s + qchunk)
        flat_list = probe[s:e].reshape(-1)
        pair_out = torch.argsort(flat_list, stable=True)
        pair_list = flat_list[pair_out].contiguous()
        pair_q = torch.div(pair_out, nprobe, rounding_mode="floor")
        part_key, part_pos = ext.ivf_scan_topk(
            Qt[s:e].contiguous(), Xs, list_off, pair_q, pair_list, pair_out,
            (e - s) * nprobe, k, mode,
        )
        part_key = part_key.view(e - s, nprobe * 64)
        part_pos = part_pos.view(e - s, nprobe * 64)
        # dead slots (lanes >= k hold -inf) and never-filled slots -> worst key
        part_key = part_key.masked_fill(part_pos < 0, float("inf"))
        vals, loc = torch.topk(part_key, k, dim=1, largest=False)
        pos = part_pos.gather(1, loc)
        keys[s:e] = vals
        ids[s:e] = torch.where(pos >= 0, order[pos.clamp(min=0)], pos)
    return keys, ids


def _dedup_topk(ids: torch.Tensor, dists: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Row-wise top-k by distance with duplicate-id suppression (duplicates
    otherwise crowd out real candidates in graph build/search)."""
    sid, order = torch.sort(ids, dim=1)
    sd = dists.gather(1, order)
    dup = torch.zeros_like(sid, dtype=torch.bool)
    dup[:, 1:] = sid[:, 1:] == sid[:, :-1]
    sd = torch.where(dup, torch.full_like(sd, 3.4e38), sd)
    vals, o2 = torch.topk(sd, min(k, sd.shape[1]), dim=1, largest=False)
    return sid.gather(1, o2), vals


def _gather_dists(A: torch.Tensor, B: torch.Tensor, cand: torch.Tensor) -> torch.Tensor:
    """d2[i][j] = ||A[i] - B[cand[i][j]]||^2 — the nn-descent / beam-search
    hot op. GPU: the `gather_dists` HIP kernel (one wave per row, A row in
    registers, candidate rows read once) replacing the torch broadcast chain
    that materializes [r, m, d] twice (reference uses
    cuVS nn_descent, umap.py:359-378)."""
    from ..ops.dispatch import has_hip_ops, hip_ops, use_hip

    if (
        A.is_cuda
        and use_hip(A, B)
        and has_hip_ops()
        and A.dtype == torch.float32
        and A.shape[1] <= 2048
    ):
        return hip_ops().gather_dists(
            A.contiguous(), B.contiguous(), cand.contiguous()
        )
    out = torch.empty(cand.shape, dtype=torch.float32, device=A.device)
    chunk = max(1, (1 << 26) // max(1, cand.shape[1] * A.shape[1]))
    for s in range(0, cand.shape[0], chunk):
        e = min(cand.shape[0], s + chunk)
        a = A[s:e][:, None, :]
        b = B[cand[s:e]]
        out[s:e] = ((a - b) ** 2).sum(dim=2)
    return out


def _batched_dists(X: torch.Tensor, rows: torch.Tensor, cand: torch.Tensor) -> torch.Tensor:
    """||X[rows][:,None] - X[cand]||^2 for cand [m, c] (chunked over m).
    Call sites pass rows = arange(n), so A = X row-aligned with cand."""
    return _gather_dists(X, X, cand)


def _reverse_edges(G: torch.Tensor, cap: int) -> torch.Tensor:
    """Per-node reverse neighbors (who points at me), capped; filler = own
    index (harmless duplicate under dedup). [n, cap] int64."""
    n, deg = G.shape
    device = G.device
    src = torch.arange(n, device=device).repeat_interleave(deg)
    dst = G.reshape(-1)
    order = torch.argsort(dst)
    dst_s = dst[order]
    src_s = src[order]
    firsts = torch.searchsorted(dst_s, torch.arange(n, device=device))
    pos = torch.arange(dst_s.numel(), device=device) - firsts[dst_s]
    keep = pos < cap
    rev = torch.arange(n, device=device)[:, None].expand(n, cap).contiguous()
    rev[dst_s[keep], pos[keep]] = src_s[keep]
    return rev


def _nn_descent(X: torch.Tensor, degree: int, n_iter: int) -> torch.Tensor:
    """Approximate kNN graph by nn-descent (reference cagra's graph build):
    start from random neighbors, iteratively propose neighbors-of-neighbors
    in BOTH directions (forward + reverse join, the core of nn-descent),
    keep the best `degree` per node. Returns [n, degree] int64."""
    n = X.shape[0]
    device = X.device
    g = torch.Generator(device="cpu")
    g.manual_seed(7)
    G = torch.randint(0, n, (n, degree), generator=g).to(device)
    rows = torch.arange(n, device=device)
    Gd = _batched_dists(X, rows, G)
    for _ in range(max(1, n_iter)):
        sub_f = G[:, : min(degree, 8)]
        rev = _reverse_edges(G, min(degree, 8))
        join = torch.cat([sub_f, rev], dim=1)  # [n, <=16]
        cand = torch.cat([G[join].reshape(n, -1), rev], dim=1)
        cd = _batched_dists(X, rows, cand)
        cat_i = torch.cat([G, cand], dim=1)
        cat_d = torch.cat([Gd, cd], dim=1)
        cat_d = torch.where(cat_i == rows[:, None], torch.full_like(cat_d, 3.4e38), cat_d)
        G, Gd = _dedup_topk(cat_i, cat_d, degree)
    return G


def _graph_beam_search(
    Qt: torch.Tensor,
    Xt: torch.Tensor,
    G: torch.Tensor,
    k: int,
    itopk: int,
    hops: int,
    expand: Optional[int] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Fixed-hop beam search over the kNN graph, vectorized over queries.
    `expand` nodes are expanded per hop (default max(4, itopk // 8))."""
    nq = Qt.shape[0]
    n = Xt.shape[0]
    device = Qt.device
    g = torch.Generator(device="cpu")
    g.manual_seed(11)
    beam = torch.randint(0, n, (nq, itopk), generator=g).to(device)
    rowsq = torch.arange(nq, device=device)

    def qdists(cand: torch.Tensor) -> torch.Tensor:
        return _gather_dists(Qt, Xt, cand)

    bd = qdists(beam)
    if expand is None:
        expand = max(4, itopk // 8)  # nodes expanded per hop
    for _ in range(hops):
        top = beam.gather(1, bd.topk(min(expand, itopk), dim=1, largest=False).indices)
        cand = G[top].reshape(nq, -1)
        cd = qdists(cand)
        cat_i = torch.cat([beam, cand], dim=1)
        cat_d = torch.cat([bd, cd], dim=1)
        beam, bd = _dedup_topk(cat_i, cat_d, itopk)

    ids2, vals2 = _dedup_topk(beam, bd, min(k, bd.shape[1]))
    return vals2, ids2  # squared-L2 keys


# -- CAGRA index: build once, query many times --------------------------------
_CAGRA_LDS_BUDGET = 144 * 1024  # cagra_search: list + candidates + filter + query
# The measured default (RESULTS.md, "CAGRA"): the kernel is the GPU search.
_CAGRA_KERNEL_DEFAULT = True


@dataclass
class CagraIndex:
    """What a graph search needs of the items, built by `_cagra_build`."""

    Xt: torch.Tensor  # [n, d] items
    G: torch.Tensor  # [n, deg] i32 search graph: forward edges, then the
    # capped reverse edges (filler = the node itself); the optimised build's
    # pruned and reverse-merged rows are exactly graph_degree wide
    G64: Optional[torch.Tensor] = None  # i64 copy, made when the torch search first runs
    seeds: Optional[torch.Tensor] = None  # [nq, itopk] i32 seeds of the last kernel search


def _cagra_build(Xt: torch.Tensor, algo_params: Dict[str, Any]) -> CagraIndex:
    """nn-descent graph of `graph_degree` forward edges, augmented with
    graph_degree // 2 reverse edges per node. With `intermediate_graph_degree`
    or `build_algo` in algoParams, cuVS's build instead: a kNN graph of the
    intermediate degree (`_cagra_knn_graph`), pruned by detour counts and
    merged with its reverse edges at exactly `graph_degree` columns
    (`_cagra_optimize`)."""
    build_iters = int(algo_params.get("nn_descent_niter", 3))
    optimize = _cagra_optimize_params(algo_params, Xt.shape[0])
    if optimize is not None:
        degree, inter, build_algo = optimize
        G = _cagra_knn_graph(Xt, inter, build_algo, build_iters)
        return CagraIndex(Xt=Xt, G=_cagra_optimize(G, degree))
    degree = int(algo_params.get("graph_degree", 32))
    G = _nn_descent(Xt, degree, build_iters)
    G_search = torch.cat([G, _reverse_edges(G, degree // 2)], dim=1)
    return CagraIndex(Xt=Xt, G=G_search.to(torch.int32).contiguous())


_CAGRA_BUILD_ALGOS = ("nn_descent", "ivf_pq")
_CAGRA_PRUNE_MAX_D = 256  # cagra_prune: widest row the kernel takes
_CAGRA_PRUNE_CHUNK_ELEMS = 1 << 22  # torch prune: rows * D * D per chunk (32 MiB of i64)


def _cagra_optimize_params(
    algo_params: Dict[str, Any], n: Optional[int] = None, warn: bool = True
) -> Optional[Tuple[int, int, str]]:
    """(graph_degree, intermediate_graph_degree, build_algo) of the optimised
    build, or None when algoParams names neither `intermediate_graph_degree`
    nor `build_algo` (the build stays as it was). The intermediate degree
    defaults to 2 * graph_degree (cuVS's 128 / 64). As in cuVS, a graph_degree
    above it is lowered to it, and with `n` given an intermediate degree >= n
    is lowered to n - 1 and graph_degree with it, each with a RuntimeWarning
    unless `warn` is off. build_algo is nn_descent (the default here; the
    reference defaults to ivf_pq, docs/parity.md) or ivf_pq, which takes an
    intermediate degree below 256 (reference knn.py:1600)."""
    if "intermediate_graph_degree" not in algo_params and "build_algo" not in algo_params:
        return None
    build_algo = algo_params.get("build_algo", "nn_descent")
    if build_algo not in _CAGRA_BUILD_ALGOS:
        raise ValueError(
            f"cagra build_algo must be 'nn_descent' or 'ivf_pq', got {build_algo!r}"
        )
    degree = int(algo_params.get("graph_degree", 32))
    inter = int(algo_params.get("intermediate_graph_degree", 2 * degree))
    if degree < 1 or inter < 1:
        raise ValueError(
            "cagra graph_degree and intermediate_graph_degree must be >= 1, got "
            f"{degree} and {inter}"
        )
    if build_algo == "ivf_pq" and inter >= 256:
        raise ValueError(
            "cagra with ivf_pq build_algo expects intermediate_graph_degree "
            f"({inter}) to be smaller than 256"
        )
    if n is not None and inter >= n:
        lowered = max(1, n - 1)
        if warn:
            warnings.warn(
                f"cagra intermediate_graph_degree ({inter}) must be below the number "
                f"of items ({n}); lowered to {lowered}",
                RuntimeWarning,
            )
        inter = lowered
    if degree > inter:
        if warn:
            warnings.warn(
                f"cagra graph_degree ({degree}) cannot exceed "
                f"intermediate_graph_degree ({inter}); lowered to {inter}",
                RuntimeWarning,
            )
        degree = inter
    return degree, inter, build_algo


def _cagra_knn_graph(Xt: torch.Tensor, degree: int, build_algo: str, n_iter: int) -> torch.Tensor:
    """The intermediate kNN graph of the optimised build, [n, degree] int64,
    each row in ascending distance order: nn-descent, or an IVF-PQ index of
    the items queried with the items themselves."""
    if build_algo == "nn_descent":
        return _nn_descent(Xt, degree, n_iter)
    return _ivfpq_knn_graph(Xt, degree)


# Build-time IVF-PQ search of `_ivfpq_knn_graph`: at normal 2000 x 16, degree
# 64, the graph's recall against the exact kNN graph was 0.28 at nlist // 16
# probed lists, 0.74 at nlist // 4 and 0.92 at nlist // 2 (RESULTS.md).
_CAGRA_IVFPQ_REFINE = 2.0


def _ivfpq_knn_graph(Xt: torch.Tensor, degree: int) -> torch.Tensor:
    """kNN graph through `_ivfpq_build` with default parameters: every item
    asks for degree + 1 neighbours over nlist // 2 probed lists with the exact
    refine, in row chunks that keep the refine's [q, k_cand, d] gather near
    1 GiB. A row drops its own id (its last entry when the search missed the
    item itself); an unfilled slot becomes the row's own id, which the prune
    treats as dead. Rows are in exact-distance order."""
    n, d = Xt.shape
    index = _ivfpq_build(Xt, {}, "sqeuclidean")
    nlist = index.boundaries.numel() - 1
    nprobe = max(1, nlist // 2)
    k = min(n, degree + 1)
    k_cand = min(n, max(k, int(k * _CAGRA_IVFPQ_REFINE)))
    chunk = max(1, (1 << 30) // (k_cand * d * 4))
    G = torch.empty((n, k - 1), dtype=torch.int64, device=Xt.device)
    cols = torch.arange(k, device=Xt.device)[None, :]
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        _, ids = _ivfpq_query(index, Xt[s:e].contiguous(), k, nprobe, _CAGRA_IVFPQ_REFINE)
        own = torch.arange(s, e, device=Xt.device)[:, None]
        is_own = ids == own
        drop = torch.where(is_own.any(dim=1), is_own.int().argmax(dim=1), k - 1)
        kept = ids[cols != drop[:, None]].view(e - s, k - 1)
        G[s:e] = torch.where(kept < 0, own, kept)
    return G


def _cagra_optimize(G: torch.Tensor, degree: int) -> torch.Tensor:
    """cuVS's graph optimisation: rank-based pruning of the intermediate graph
    to `degree` columns, then the reverse-edge merge. [n, degree] i32."""
    P, _ = _cagra_prune(G, degree)
    return _cagra_merge_reverse(P).to(torch.int32).contiguous()


def _cagra_prune_kernel_wanted(G: torch.Tensor) -> bool:
    """Route the pruning through the `cagra_prune` kernel? On the GPU, for
    rows of at most 256 ids. SRML_CAGRA_PRUNE_KERNEL=0 forces the torch
    formulation. On a GPU without the built extension the kernel path raises,
    as every HIP path."""
    from ..ops.dispatch import use_hip

    if os.environ.get("SRML_CAGRA_PRUNE_KERNEL") == "0":
        return False
    if not (G.is_cuda and use_hip(G)):
        return False
    return G.shape[1] <= _CAGRA_PRUNE_MAX_D and G.shape[0] < 2**31


def _cagra_prune(G: torch.Tensor, d_out: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Rank-based detour pruning of a kNN graph G [n, D] whose rows are in
    ascending distance order. Entry j of row u is dead if it is u itself or
    repeats an earlier entry; a live j has
    detour[u][j] = #{i < j : i live and G[u][j] in set(G[G[u][i]])}, a dead
    one -1. P[u] is the live entries by (detour, j), cut to d_out and padded
    with u. Integer-only, the same on the kernel and the torch path.
    Returns (P [n, d_out] int64, detour [n, D] int32)."""
    n, D = G.shape
    if not 1 <= d_out <= D:
        raise ValueError(f"cagra prune needs 1 <= D_out <= D, got {d_out} and {D}")
    if _cagra_prune_kernel_wanted(G):
        from ..ops.dispatch import hip_ops

        P, detour = hip_ops().cagra_prune(G.to(torch.int32).contiguous(), d_out)
        return P.to(torch.int64), detour
    G = G.to(torch.int64)
    device = G.device
    P = torch.empty((n, d_out), dtype=torch.int64, device=device)
    detour = torch.empty((n, D), dtype=torch.int32, device=device)
    before = torch.ones((D, D), dtype=torch.bool, device=device).triu(1)  # [i, j]: i < j
    ranks = torch.arange(D, device=device)
    # the [rows, D, D] neighbour-row gather and its searchsorted temporaries
    chunk = max(1, _CAGRA_PRUNE_CHUNK_ELEMS // (D * D))
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        ids = G[s:e]
        own = torch.arange(s, e, device=device)[:, None]
        sid, order = torch.sort(ids, dim=1, stable=True)
        dup_s = torch.zeros_like(sid, dtype=torch.bool)
        dup_s[:, 1:] = sid[:, 1:] == sid[:, :-1]
        dup = torch.zeros_like(dup_s).scatter_(1, order, dup_s)
        live = ~dup & (ids != own)
        # hit[r, i, j]: G[u][j] occurs in neighbour i's raw row
        nbr = torch.sort(G[ids], dim=2).values  # [r, D(i), D]
        want = ids[:, None, :].expand(-1, D, -1).contiguous()  # [r, D(i), D(j)]
        at = torch.searchsorted(nbr, want).clamp(max=D - 1)
        hit = nbr.gather(2, at) == want
        hit &= live[:, :, None] & before[None]
        cnt = hit.sum(dim=1).to(torch.int32)
        cnt = torch.where(live, cnt, torch.full_like(cnt, -1))
        detour[s:e] = cnt
        key = torch.where(live, cnt.to(torch.int64) * 512 + ranks, 1 << 40)
        skey, sel = torch.sort(key, dim=1)
        picked = ids.gather(1, sel[:, :d_out])
        P[s:e] = torch.where(skey[:, :d_out] < (1 << 40), picked, own)
    return P, detour


def _cagra_merge_reverse(P: torch.Tensor) -> torch.Tensor:
    """Reverse-edge merge of a pruned graph P [n, D_out] (filler = the row's
    own id). Edges u -> P[u][k] are taken in (k, u) order, so the strongest
    edges claim a node's reverse slots first; rev[v] is the first D_out
    sources that reach v. F[u] is the first D_out distinct ids other than u
    of P[u][:D_out // 2] ++ rev[u] ++ P[u][D_out // 2:], padded with u.
    Returns F [n, D_out] int64."""
    n, d_out = P.shape
    P = P.to(torch.int64)
    device = P.device
    h = d_out // 2
    own = torch.arange(n, device=device)
    dst = P.t().reshape(-1)  # (k, u) order
    src = own.repeat(d_out)
    real = dst != src
    dst, src = dst[real], src[real]
    order = torch.argsort(dst, stable=True)
    dst_s, src_s = dst[order], src[order]
    firsts = torch.searchsorted(dst_s, own)
    pos = torch.arange(dst_s.numel(), device=device) - firsts[dst_s]
    keep = pos < d_out
    rev = own[:, None].repeat(1, d_out)  # a copy also at d_out = 1
    rev[dst_s[keep], pos[keep]] = src_s[keep]
    cat = torch.cat([P[:, :h], rev, P[:, h:]], dim=1)  # [n, 2 * d_out]
    # first occurrence of every id other than the row's own, in column order
    sid, order = torch.sort(cat, dim=1, stable=True)
    dup_s = torch.zeros_like(sid, dtype=torch.bool)
    dup_s[:, 1:] = sid[:, 1:] == sid[:, :-1]
    dup = torch.zeros_like(dup_s).scatter_(1, order, dup_s)
    good = ~dup & (cat != own[:, None])
    cols = torch.arange(cat.shape[1], device=device)[None, :]
    skey, sel = torch.sort(torch.where(good, cols, cat.shape[1]), dim=1)
    picked = cat.gather(1, sel[:, :d_out])
    return torch.where(skey[:, :d_out] < cat.shape[1], picked, own[:, None])


def _cagra_search_params(algo_params: Dict[str, Any], k: int) -> Tuple[int, int, int]:
    """(itopk_size, search_width, max_iterations) of a search for k.
    itopk_size defaults to max(64, 2k) and is rounded up to a multiple of 32,
    as cuVS does; below k it is an error (reference knn.py:1350-1359).
    search_width defaults to max(4, itopk_size // 8), not cuVS's 1: at width 1
    ten iterations reach too few nodes (docs/parity.md). max_iterations absent
    or 0 means ceil(itopk_size / search_width) + 10; the search stops by
    itself once every kept entry has been expanded."""
    itopk = int(algo_params.get("itopk_size", max(64, 2 * k)))
    itopk = max(32, math.ceil(itopk / 32) * 32)
    if itopk < k:
        raise ValueError(
            "cagra increases itopk_size to be closest multiple of 32 and expects "
            f"the value, i.e. {itopk}, to be larger than or equal to k, i.e. {k})."
        )
    width = int(algo_params.get("search_width", max(4, itopk // 8)))
    if width < 1:
        raise ValueError(f"search_width must be >= 1, got {width}")
    max_it = int(algo_params.get("max_iterations", 0) or 0)
    if max_it <= 0:
        max_it = math.ceil(itopk / width) + 10
    return itopk, width, max_it


def _cagra_kernel_wanted(
    index: CagraIndex, Qt: torch.Tensor, k: int, itopk: int, width: int
) -> bool:
    """Route the graph search through the `cagra_search` kernel? On the GPU,
    for f32 inputs within the wrapper's limits (k <= itopk <= 512, d <= 2048,
    deg <= 128, search_width * deg <= 2048, its LDS budget).
    SRML_CAGRA_KERNEL=0 forces the torch search; =1 asks for the kernel, which
    it gets wherever it is legal; unset takes the measured default. On a GPU
    without the built extension the kernel path raises, as every HIP path."""
    from ..ops.dispatch import use_hip

    env = os.environ.get("SRML_CAGRA_KERNEL")
    if env == "0" or not (Qt.is_cuda and use_hip(Qt, index.Xt)):
        return False
    if Qt.dtype != torch.float32 or index.Xt.dtype != torch.float32:
        return False
    n, d = index.Xt.shape
    deg = index.G.shape[1]
    if not (1 <= k <= itopk <= 512 and 1 <= d <= 2048 and 1 <= deg <= 128):
        return False
    if width * deg > 2048 or n >= 2**31:
        return False
    slots = _pow2_ceil(2 * (itopk + width * deg))
    lds = (
        _pow2_ceil(itopk + width * deg) * 8
        + slots * 4
        + (min(width, itopk) + 3) // 4 * 16
        + (d + 3) // 4 * 16
    )
    if lds > _CAGRA_LDS_BUDGET:
        return False
    return env == "1" or _CAGRA_KERNEL_DEFAULT


def _cagra_query(
    index: CagraIndex, Qt: torch.Tensor, k: int, itopk: int, width: int, max_it: int
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Search the kept graph from itopk random seeds per query (CPU generator,
    seed 11, the same on both paths). Returns (squared-L2 keys, item rows):
    the fused kernel where `_cagra_kernel_wanted` says so, with (+inf, -1) in
    slots it could not fill, `_graph_beam_search` otherwise."""
    if not _cagra_kernel_wanted(index, Qt, k, itopk, width):
        if index.G64 is None:  # torch indexing wants i64: cast once, not per call
            index.G64 = index.G.to(torch.int64)
        return _graph_beam_search(Qt, index.Xt, index.G64, k, itopk, max_it, expand=width)
    keys, ids, _ = _cagra_search_kernel(index, Qt, k, itopk, width, max_it)
    return keys, ids.to(torch.int64)


def _cagra_search_kernel(
    index: CagraIndex, Qt: torch.Tensor, k: int, itopk: int, width: int, max_it: int
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Kernel path of `_cagra_query`: one block per query, the whole search
    in one launch. Returns (keys, i32 item rows, stats [nq, 3] = iterations,
    distance evaluations, visited-filter resets per query)."""
    from ..ops.dispatch import hip_ops

    nq, n = Qt.shape[0], index.Xt.shape[0]
    seeds = index.seeds
    # the seeds depend on (nq, itopk) alone: repeated calls of one shape reuse them
    if seeds is None or tuple(seeds.shape) != (nq, itopk) or seeds.device != Qt.device:
        g = torch.Generator(device="cpu")
        g.manual_seed(11)
        seeds = torch.randint(0, n, (nq, itopk), generator=g).to(torch.int32).to(Qt.device)
        index.seeds = seeds
    return hip_ops().cagra_search(
        Qt.contiguous(), index.Xt.contiguous(), index.G, seeds, k, itopk, width, max_it, 0
    )


def _pq_encode(resid: torch.Tensor, m_sub: int, n_codes: int = 256, iters: int = 8):
    """Train per-subspace codebooks (k-means on a sample) and encode.
    Returns (codebooks [m, n_codes, ds], codes uint8 [n, m])."""
    n, d = resid.shape
    ds = d // m_sub
    device = resid.device
    g = torch.Generator(device="cpu")
    g.manual_seed(123)
    n_codes = min(n_codes, max(2, n))
    sample = resid[torch.randperm(n, generator=g)[: min(n, 65536)].to(device)]
    codebooks = torch.empty(m_sub, n_codes, ds, dtype=torch.float32, device=device)
    codes = torch.empty(n, m_sub, dtype=torch.uint8, device=device)
    for m in range(m_sub):
        sub = sample[:, m * ds : (m + 1) * ds].contiguous()
        cb = sub[torch.randperm(sub.shape[0], generator=g)[:n_codes].to(device)].clone()
        for _ in range(iters):
            d2 = (
                (sub * sub).sum(1)[:, None]
                + (cb * cb).sum(1)[None, :]
                - 2.0 * (sub @ cb.T)
            )
            lb = d2.argmin(dim=1)
            sums = torch.zeros_like(cb)
            cnt = torch.zeros(n_codes, device=device)
            sums.index_add_(0, lb, sub)
            cnt.index_add_(0, lb, torch.ones_like(lb, dtype=torch.float32))
            ne = cnt > 0
            cb[ne] = sums[ne] / cnt[ne, None]
        codebooks[m] = cb
        full = resid[:, m * ds : (m + 1) * ds]
        # chunked encode
        for s0 in range(0, n, 1 << 18):
            e0 = min(n, s0 + (1 << 18))
            d2 = (
                (full[s0:e0] * full[s0:e0]).sum(1)[:, None]
                + (cb * cb).sum(1)[None, :]
                - 2.0 * (full[s0:e0] @ cb.T)
            )
            codes[s0:e0, m] = d2.argmin(dim=1).to(torch.uint8)
    return codebooks, codes


def _ivfpq_scan(
    Qt: torch.Tensor,
    C: torch.Tensor,
    labels: torch.Tensor,
    codebooks: torch.Tensor,
    codes: torch.Tensor,
    nlist: int,
    nprobe: int,
    k: int,
    mode: int = _MODE_L2,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """ADC scan: per (query, probed list), approx dist = ||q - c_list||-part
    + sum_m LUT[m, code_m] where LUT holds ||(q - c_list)_m - cb[m,j]||².
    mode 1 (dot-product key): -(q.c_list + sum_m q_m.cb[m, code_m]) — the
    LUT holds the dots of the query itself, there is no residual query."""
    device = Qt.device
    nq = Qt.shape[0]
    m_sub, n_codes, ds = codebooks.shape
    nprobe = min(nprobe, nlist)
    probe = _probe_lists(Qt, C, nprobe, mode)  # [nq, nprobe]

    order = torch.argsort(labels)
    sorted_labels = labels[order]
    boundaries = torch.searchsorted(
        sorted_labels, torch.arange(nlist + 1, device=device)
    )
    best_d = torch.full((nq, k), float("inf"), device=device)
    best_i = torch.full((nq, k), -1, dtype=torch.int64, device=device)
    cb_sq = (codebooks * codebooks).sum(dim=2)  # [m, 256]
    for p in range(nprobe):
        lists = probe[:, p]  # per-query probed list id
        # group queries by list for batched LUT scans
        uniq, inv = torch.unique(lists, return_inverse=True)
        for ui in range(uniq.numel()):
            l = int(uniq[ui])
            s, e = int(boundaries[l]), int(boundaries[l + 1])
            if s == e:
                continue
            qsel = torch.nonzero(inv == ui).flatten()
            items = order[s:e]
            if mode == _MODE_DOT:
                qb = Qt[qsel]
                qr = qb.reshape(-1, m_sub, ds)
                lut = -torch.einsum("qmd,mcd->qmc", qr, codebooks)
                base = -(qb @ C[l])  # [m_q]
            else:
                qres = Qt[qsel] - C[l][None, :]  # [m_q, d] residual queries
                # LUT [m_q, m_sub, 256]: ||qres_m||² - 2 qres_m . cb + ||cb||²
                qr = qres.view(-1, m_sub, ds)
                dots = torch.einsum("qmd,mcd->qmc", qr, codebooks)
                lut = (qr * qr).sum(2)[:, :, None] - 2.0 * dots + cb_sq[None, :, :]
                base = None
            lc = codes[items].long()  # [n_l, m_sub]
            # approx dists [m_q, n_l] = sum_m lut[q, m, code]
            d_apx = torch.zeros(qsel.numel(), items.numel(), device=device)
            if base is not None:
                d_apx += base[:, None]
            for m in range(m_sub):
                d_apx += lut[:, m, :].gather(
                    1, lc[:, m][None, :].expand(qsel.numel(), -1)
                )
            kb = min(k, items.numel())
            vals, loc = torch.topk(d_apx, kb, dim=1, largest=False)
            ids = items[loc]
            cat_d = torch.cat([best_d[qsel], vals], dim=1)
            cat_i = torch.cat([best_i[qsel], ids], dim=1)
            mvals, morder = torch.topk(cat_d, k, dim=1, largest=False)
            rows = torch.arange(qsel.numel(), device=device)[:, None]
            best_d[qsel] = mvals
            best_i[qsel] = cat_i.gather(1, morder)
    return best_d, best_i


# -- IVF-PQ index: build once, query many times -------------------------------
_PQ_LDS_BUDGET = 144 * 1024  # ivfpq_scan_topk: LUT + query + merge buffer


@dataclass
class IvfPqIndex:
    """What an IVF-PQ search needs of the items, built by `_ivfpq_build`."""

    Xt: torch.Tensor  # [n, d] items (unit rows for cosine), for the refine
    C: torch.Tensor  # [nlist, d] coarse centres
    labels: torch.Tensor  # [n] list of each item
    order: torch.Tensor  # [n] item rows sorted by list
    boundaries: torch.Tensor  # [nlist + 1] list offsets into `order`
    codebooks: torch.Tensor  # [M, ncodes, ds]
    codes: torch.Tensor  # [n, M] u8, item order
    codes_sorted: torch.Tensor  # [n, M padded to a multiple of 4] u8, list order
    m_sub: int
    n_bits: int
    mode: int


def _ivfpq_n_bits(algo_params: Dict[str, Any]) -> int:
    """algoParams["n_bits"] (reference ivfpq algoParams: nlist, nprobe, M,
    n_bits): bits per code, an integer 4..8, default 8."""
    n_bits = algo_params.get("n_bits", 8)
    ok = isinstance(n_bits, (int, np.integer)) and not isinstance(n_bits, bool)
    if not ok or not 4 <= int(n_bits) <= 8:
        raise ValueError(f"n_bits must be an integer from 4 to 8, got {n_bits!r}")
    return int(n_bits)


def _ivfpq_build(Xt: torch.Tensor, algo_params: Dict[str, Any], metric: str) -> IvfPqIndex:
    """Coarse k-means, residual codebooks of 2**n_bits codes per subspace
    and the one-byte codes, in item order and in list order."""
    n_bits = _ivfpq_n_bits(algo_params)
    if metric == "cosine":
        Xt = _normalize_rows(Xt)
    n, d = Xt.shape
    nlist = int(algo_params.get("nlist", _default_nlist(n)))
    m_sub = int(algo_params.get("M", max(1, d // 4)))
    while d % m_sub != 0:  # subspace dims must divide d
        m_sub -= 1
    C, labels = _build_coarse(Xt, nlist)
    resid = Xt - C[labels]
    codebooks, codes = _pq_encode(resid, m_sub, n_codes=2**n_bits)
    order = torch.argsort(labels)
    boundaries = torch.searchsorted(
        labels[order], torch.arange(nlist + 1, device=Xt.device)
    )
    # the kernel reads a row's codes as dwords: pad the list-sorted rows to a
    # multiple of 4 bytes (the pad columns are never used as codes)
    codes_sorted = torch.zeros(
        (n, (m_sub + 3) // 4 * 4), dtype=torch.uint8, device=Xt.device
    )
    codes_sorted[:, :m_sub] = codes[order]
    return IvfPqIndex(
        Xt=Xt, C=C, labels=labels, order=order, boundaries=boundaries,
        codebooks=codebooks, codes=codes, codes_sorted=codes_sorted,
        m_sub=m_sub, n_bits=n_bits, mode=_metric_mode(metric),
    )


def _ivfpq_query(
    index: IvfPqIndex, Qt: torch.Tensor, k: int, nprobe: int, refine_ratio: float
) -> Tuple[torch.Tensor, torch.Tensor]:
    """ADC scan for k*refine_ratio candidates, then the exact re-rank.
    `Qt` is already normalised for cosine. Returns (keys, item rows)."""
    Xt, mode = index.Xt, index.mode
    n = Xt.shape[0]
    k_cand = min(n, max(k, int(k * refine_ratio)))
    _, i_c = _ivfpq_candidates(index, Qt, nprobe, k_cand)
    # exact refine on candidates (full-precision vectors resident)
    rows = torch.arange(Qt.shape[0], device=Qt.device)[:, None]
    cand = Xt[i_c.clamp(min=0)]  # [q, k_cand, d]
    if mode == _MODE_DOT:
        d_exact = -(Qt[:, None, :] * cand).sum(dim=2)
    else:
        d_exact = ((Qt[:, None, :] - cand) ** 2).sum(dim=2)
    d_exact = torch.where(i_c >= 0, d_exact, torch.full_like(d_exact, float("inf")))
    vals, order = torch.topk(d_exact, min(k, k_cand), dim=1, largest=False)
    return vals, i_c[rows, order]


def _ivfpq_candidates(
    index: IvfPqIndex, Qt: torch.Tensor, nprobe: int, k_cand: int
) -> Tuple[torch.Tensor, torch.Tensor]:
    """The k_cand best ADC keys per query over its probed lists and their
    item rows (+inf, -1 for an empty slot): the fused kernel where
    `_ivfpq_kernel_wanted` says so, the torch scan otherwise."""
    if _ivfpq_kernel_wanted(index, Qt, k_cand):
        return _ivfpq_scan_kernel(index, Qt, nprobe, k_cand)
    nlist = index.boundaries.numel() - 1
    return _ivfpq_scan(
        Qt, index.C, index.labels, index.codebooks, index.codes,
        nlist, nprobe, k_cand, index.mode,
    )


def _pow2_ceil(v: int) -> int:
    return 1 << max(0, int(v) - 1).bit_length()


def _ivfpq_slots(k_cand: int) -> int:
    """Slots per pair the kernel writes: 64 * SLOTS, SLOTS in {1, 2, 4}."""
    return 64 if k_cand <= 64 else (128 if k_cand <= 128 else 256)


def _ivfpq_kernel_wanted(index: IvfPqIndex, Qt: torch.Tensor, k_cand: int) -> bool:
    """Route the ADC scan through the `ivfpq_scan_topk` kernel? On the GPU,
    for f32 inputs, k_cand <= 256 and a lookup table that fits the kernel's
    LDS budget. SRML_IVFPQ_KERNEL=0 forces the
    torch scan; =1 asks for the kernel, which it gets wherever it is legal."""
    from ..ops.dispatch import use_hip

    env = os.environ.get("SRML_IVFPQ_KERNEL")
    if env == "0" or not (Qt.is_cuda and use_hip(Qt, index.Xt)):
        return False
    if Qt.dtype != torch.float32 or index.C.dtype != torch.float32:
        return False
    m_sub, n_codes, _ = index.codebooks.shape
    d = Qt.shape[1]
    if not 1 <= k_cand <= 256 or n_codes > 256:
        return False
    if index.C.shape[0] != index.boundaries.numel() - 1:  # nlist > n
        return False
    lds = m_sub * _pow2_ceil(n_codes) * 4 + (d + 3) // 4 * 16 + 3 * _ivfpq_slots(k_cand) * 8
    if lds > _PQ_LDS_BUDGET:
        return False
    return True


def _ivfpq_scan_kernel(
    index: IvfPqIndex, Qt: torch.Tensor, nprobe: int, k_cand: int
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Kernel path of the ADC scan, same results as `_ivfpq_scan`: one block
    per (query, probed list) pair builds the pair's lookup table in LDS and
    keeps the list's k_cand best rows in 64*SLOTS slots, then one topk over
    each query's nprobe*64*SLOTS slots. Pairs are sorted by list, as in
    `_ivf_scan_kernel`, so neighbouring blocks stream the same code rows."""
    from ..ops.dispatch import hip_ops

    ext = hip_ops()
    mode = index.mode
    nlist = index.boundaries.numel() - 1
    nprobe = min(nprobe, nlist)
    probe = _probe_lists(Qt, index.C, nprobe, mode)  # [nq, nprobe]
    nq = Qt.shape[0]
    slots = _ivfpq_slots(k_cand)
    order = index.order
    list_off = index.boundaries.to(torch.int64).contiguous()
    codebooks = index.codebooks
    m_sub, n_codes, ds = codebooks.shape
    if n_codes & (n_codes - 1):
        # fewer items than 2**n_bits leave a short codebook: the kernel masks
        # codes with a power of two, so pad with rows no code refers to
        pad = codebooks.new_zeros((m_sub, _pow2_ceil(n_codes) - n_codes, ds))
        codebooks = torch.cat([codebooks, pad], dim=1).contiguous()
    keys = torch.empty((nq, k_cand), dtype=torch.float32, device=Qt.device)
    ids = torch.empty((nq, k_cand), dtype=torch.int64, device=Qt.device)
    # key (f32) + position (i64) slot buffers stay under 512 MB per chunk
    qchunk = max(1, (512 << 20) // (nprobe * slots * 12))
    for s in range(0, nq, qchunk):
        e = min(nq, s + qchunk)
        flat_list = probe[s:e].reshape(-1)
        pair_out = torch.argsort(flat_list, stable=True)
        pair_list = flat_list[pair_out].contiguous()
        pair_q = torch.div(pair_out, nprobe, rounding_mode="floor")
        part_key, part_pos = ext.ivfpq_scan_topk(
            Qt[s:e].contiguous(), index.C.contiguous(), codebooks,
            index.codes_sorted, list_off, pair_q, pair_list, pair_out,
            (e - s) * nprobe, k_cand, mode,
        )
        part_key = part_key.view(e - s, nprobe * slots)
        part_pos = part_pos.view(e - s, nprobe * slots)
        # dead slots (-inf) and never-filled slots -> worst key
        part_key = part_key.masked_fill(part_pos < 0, float("inf"))
        vals, loc = torch.topk(part_key, k_cand, dim=1, largest=False)
        pos = part_pos.gather(1, loc)
        keys[s:e] = vals
        ids[s:e] = torch.where(pos >= 0, order[pos.clamp(min=0)], pos)
    return keys, ids
