"""Regenerate docs/api.md from the live param system.

Usage: python tools/gen_api_doc.py
"""
import sys
import warnings

warnings.filterwarnings("ignore")
sys.path.insert(0, ".")

import spark_rapids_ml_amd as pkg  # noqa: E402

CLASSES = [
    "KMeans", "KMeansModel", "DBSCAN", "DBSCANModel", "PCA", "PCAModel",
    "LinearRegression", "LinearRegressionModel",
    "LogisticRegression", "LogisticRegressionModel",
    "RandomForestClassifier", "RandomForestClassificationModel",
    "RandomForestRegressor", "RandomForestRegressionModel",
    "NearestNeighbors", "ApproximateNearestNeighbors",
    "UMAP", "UMAPModel",
]

TAIL = """## Metrics

`ApproximateNearestNeighbors(metric=...)` / `setMetric` / `getMetric` \
(reference knn.py:1007-1010). An unknown name raises `ValueError` from \
`setMetric`, and from `kneighbors` when it came in through the constructor.

| metric | ivfflat | ivfpq | cagra | `distances` column | order | empty slot |
|---|---|---|---|---|---|---|
| `euclidean`, `l2` | yes | yes | yes | L2 distance | ascending | `+inf`, id `-1` |
| `sqeuclidean` | yes | yes | yes | squared L2 distance | ascending | `+inf`, id `-1` |
| `cosine` | yes | yes | `ValueError` | `1 - cos` | ascending | `+inf`, id `-1` |
| `inner_product` | yes | yes | `ValueError` | raw dot product `q.x` | descending | `-inf`, id `-1` |

`cosine` normalises every row by `max(norm, 1e-30)`: a zero vector stays \
zero and comes out at cosine distance 0.5 from everything. An empty slot \
appears when fewer than `k` items are reachable through the probed lists \
(or, for cagra, through the graph). \
Exact `NearestNeighbors` has no metric parameter (Euclidean, as in the \
reference).

`algoParams` of `algorithm="ivfpq"` (the reference's four, plus the refine):

| key | default | meaning |
|---|---|---|
| `nlist` | `min(1024, sqrt(n))` | coarse lists |
| `nprobe` | `max(1, nlist // 16)` | lists scanned per query |
| `M` | `d // 4`, lowered until it divides `d` | subquantizers |
| `n_bits` | 8 | bits per code: an integer 4..8, `2**n_bits` codes per subquantizer, one byte per code; anything else raises `ValueError` naming `n_bits` |
| `refine_ratio` | 2.0 | `k * refine_ratio` ADC candidates (at most `n`) are re-ranked by the true metric |

An ivfpq model builds its index (coarse k-means, codebooks, codes) in the \
first `kneighbors` call and keeps it: a later call with the same \
(`algorithm`, `algoParams`, `metric`) only searches and returns bit-identical \
results for the same queries; a changed key rebuilds. One index is kept per \
model and per rank. `SRML_ANN_CACHE=0` builds on every call. On the GPU the \
ADC scan runs the `ivfpq_scan_topk` kernel (f32, `k * refine_ratio <= 256`, \
`M * 2**n_bits * 4` bytes of lookup table within the 144 KB LDS budget, i.e. \
`M <= 128` at 8 bits); `SRML_IVFPQ_KERNEL=0` forces the torch scan, which \
also serves every case the kernel does not take.

ivfflat keeps its coarse index (`nlist` k-means lists) the same way, under \
`nlist` and the metric; `nprobe` is a search parameter and never rebuilds.

`algoParams` of `algorithm="cagra"`:

| key | default | meaning |
|---|---|---|
| `graph_degree` | 32 | forward edges per node of the nn-descent graph; `graph_degree // 2` reverse edges are appended (build) |
| `nn_descent_niter` | 3 | nn-descent rounds (build) |
| `intermediate_graph_degree` | absent; `2 * graph_degree` once `build_algo` is given | present (or with `build_algo`): the optimised build. A kNN graph of this many edges per node is pruned by rank-based detour counts to `graph_degree` columns and merged with its reverse edges, so the search graph is exactly `graph_degree` wide. A `graph_degree` above it is lowered to it, and a value `>= n` is lowered to `n - 1` (and `graph_degree` with it), each with a `RuntimeWarning` (build) |
| `build_algo` | absent; `"nn_descent"` once `intermediate_graph_degree` is given | `"nn_descent"` or `"ivf_pq"` (an IVF-PQ index of the items with default parameters, queried with the items over `nlist // 2` lists with refine ratio 2); anything else raises `ValueError`. `"ivf_pq"` with `intermediate_graph_degree >= 256` raises the reference's `ValueError`. The reference defaults to `"ivf_pq"` (docs/parity.md) (build) |
| `compression` | - | not supported: the key is ignored, the items stay f32 |
| `itopk_size` | `max(64, 2k)` | entries kept during the search; rounded up to a multiple of 32, and a rounded value below `k` raises `ValueError` before any work (reference knn.py:1350-1359) |
| `search_width` | `max(4, itopk_size // 8)` | entries expanded per iteration. cuVS defaults to 1; at width 1 and 10 iterations recall@10 at 20000x64 falls to 0.63, so the default stays the width the search has always used |
| `max_iterations` | 0 | 0 or absent: `ceil(itopk_size / search_width) + 10`; the search stops earlier once every kept entry has been expanded |

A cagra model builds its graph in the first `kneighbors` call and keeps it \
under `graph_degree` and `nn_descent_niter` (and the metric), plus the \
resolved `intermediate_graph_degree` and `build_algo` when either is given: \
changing `itopk_size`, `search_width` or `max_iterations` between calls never \
rebuilds. With neither of the two keys the build is the one it has always \
been (`graph_degree` forward + `graph_degree // 2` reverse columns). In the \
optimised build the pruning is the `cagra_prune` kernel on the GPU (rows of \
at most 256 ids; `SRML_CAGRA_PRUNE_KERNEL=0` forces the torch formulation, \
which gives the same integers and serves the CPU); the reverse-edge merge is \
torch on both devices. On the GPU \
the search is the `cagra_search` kernel (f32, `k <= itopk_size <= 512`, \
`d <= 2048`, graph rows of at most 128 entries, `search_width * row <= 2048`): \
one block per query keeps the itopk list, the candidates and a visited filter \
in LDS, keys every node once per filter period and never re-expands a node. \
`SRML_CAGRA_KERNEL=0` forces the torch beam search, which also serves the \
CPU and every case outside those limits with the same parameters. Slots the \
search could not fill report id `-1` and `+inf`.

`DBSCAN(metric=...)` (reference clustering.py:761):

| metric | meaning |
|---|---|
| `euclidean` | `eps` bounds the L2 distance |
| `cosine` | `eps` bounds `1 - cos`; a zero-norm row raises `ValueError` |

Any other DBSCAN metric raises `ValueError` at `transform`.

`UMAP(metric=..., metric_kwds={"p": ...})` (reference umap.py metric list). Only the kNN stage of fit and transform depends on the metric; a fitted model keeps its estimator's `metric` / `metric_kwds` (also through save / load) and transforms with them. All errors are `ValueError`.

| metric (aliases) | distance | kNN path on the GPU | `build_algo="nn_descent"` |
|---|---|---|---|
| `euclidean` (`l2`) | √Σ(x−y)² | library GEMM + `knn_merge_topk` (unchanged) | yes |
| `sqeuclidean` | Σ(x−y)² | same, no final sqrt | yes |
| `cosine` | 1 − x·y/(‖x‖‖y‖) | GEMM on unit rows; a zero-norm row raises | yes, on the unit rows |
| `correlation` | cosine of the mean-centred rows | GEMM; a constant row raises | yes, on the centred unit rows |
| `hellinger` | √max(0, 1 − Σ√(xᵢyᵢ)) | GEMM on √x rows; a negative entry raises | raises |
| `manhattan` (`l1`, `cityblock`, `taxicab`) | Σ\\|x−y\\| | `pairwise_dist` + `knn_merge_topk_keys` | raises |
| `chebyshev` (`linf`) | max\\|x−y\\| | same | raises |
| `minkowski` | (Σ\\|x−y\\|ᵖ)^(1/p), `p` from `metric_kwds` (default 2; finite and > 0; 1 and 2 resolve to manhattan and euclidean) | same | raises |
| `canberra` | Σ\\|x−y\\|/(\\|x\\|+\\|y\\|), 0/0 = 0 | same | raises |
| `hamming` | (#coordinates with xᵢ≠yᵢ)/d | same | raises |
| `jaccard` | 1 − \\|nz(x)∩nz(y)\\|/\\|nz(x)∪nz(y)\\| of the stored-entry patterns, 0 for two empty rows | sparse input only (below); dense input raises `Metric 'jaccard' not supported for dense inputs.` | raises |

Under `build_algo="auto"` the per-coordinate metrics and hellinger build the graph by brute force at any size; the L2-reducible ones switch to nn-descent above 50 000 rows as euclidean does. An unknown name raises and lists the accepted names.

Sparse input. A scipy CSR feature column stays CSR (`enable_sparse_data_optim`: `None` follows the input, `True` requires CSR, `False` densifies as before). The graph is then built by `ops/knn.py::knn_topk_metric_sparse`: per item chunk a CSC is built in torch and the `csr_pairwise` HIP kernel walks only the stored entries of both sides, `knn_merge_topk_keys` keeps the running top-k. Every metric above except `chebyshev`/`linf` and `correlation` is accepted, plus `jaccard`; those two and `build_algo="nn_descent"` raise a `ValueError` naming "sparse input" (`auto` means brute force). `UMAPModel.rawData` is then a `scipy.sparse.csr_matrix`, persisted as its three arrays and shape; `transform` takes a CSR batch as is and converts a dense one.

## Evaluators

`RegressionEvaluator` (rmse|mse|r2|mae|var), `MulticlassClassificationEvaluator` \
(f1|accuracy|weighted*|hammingLoss|logLoss + *ByLabel metrics via `metricLabel`), \
`BinaryClassificationEvaluator` (areaUnderROC|areaUnderPR).

## Tuning & Pipeline

`CrossValidator(estimator, estimatorParamMaps, evaluator, numFolds, seed, \
collectSubModels)` with single-pass `fitMultiple` and save/load; \
`ParamGridBuilder`; `Pipeline`/`PipelineModel` with the VectorAssembler \
bypass and save/load; `VectorAssembler`, `NoOpTransformer`.

## CLI entry points

| command | purpose |
|---|---|
| `srml-amd-run app.py` (= `python -m spark_rapids_ml_amd app.py`) | run a reference-style script unmodified: installs the `spark_rapids_ml` aliases, initializes the communicator |
| `srml-amd-launch [--gpus N] app.py` | spark-submit analog: execs torchrun with one rank per visible GPU, routing the script through the runner above |
| `srml-amd-server --port 8571` | remote fit/transform HTTP service (Spark Connect plugin analog) |
| `srml-amd-install` | print/emit the no-import-change alias setup |

All estimators, models, `Pipeline`/`PipelineModel`, `CrossValidator`/
`CrossValidatorModel` support `save(path)` / `.load(path)` (and
`.write().overwrite().save()`); models persist as `metadata.json` +
`attributes.npz` (+`attributes.json`).
"""


def fmt_default(inst, p):
    if not inst.hasDefault(p):
        return "—"
    v = inst.getOrDefault(p.name)
    return "None" if v is None else str(v)


def main() -> None:
    lines = ["# API reference (generated from the live param system)", ""]
    for name in CLASSES:
        cls = getattr(pkg, name)
        lines.append(f"## {name}")
        lines.append("")
        doc = (cls.__doc__ or "").strip().splitlines()
        if doc:
            lines.append(doc[0].strip())
            lines.append("")
        try:
            inst = cls()
        except Exception:
            inst = None
        if inst is not None and inst.params:
            mapping = cls._param_mapping() if hasattr(cls, "_param_mapping") else {}
            lines.append("| Spark param | default | native param |")
            lines.append("|---|---|---|")
            for p in inst.params:
                native = mapping.get(p.name, p.name)
                if native is None:
                    native = "*(unsupported: raises)*"
                elif native == "":
                    native = "*(accepted, no native effect)*"
                lines.append(f"| {p.name} | {fmt_default(inst, p)} | {native} |")
            lines.append("")
    lines.append(TAIL)
    with open("docs/api.md", "w") as f:
        f.write("\n".join(lines))
    print("docs/api.md regenerated")


if __name__ == "__main__":
    main()
