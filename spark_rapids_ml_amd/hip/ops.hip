// Hand-written CDNA4 (gfx950) kernels for spark_rapids_ml_amd.
//
// These replace the cuML/RAFT native layer of the reference:
// - kmeans_assign: fused pairwise-distance (MFMA f32) + argmin, the KMeansMG
//   Lloyd-step hot kernel (reference clustering.py:381-415 call site).
// - gram_f32: X^T X partials on MFMA f32 — PCAMG covariance
//   (feature.py:232-253) and LinearRegressionMG normal equations
//   (regression.py:549) building block.
// - softmax_residual_loss: fused softmax/sigmoid + residual + loss for the
//   LogisticRegressionMG L-BFGS iteration (classification.py:1046-1081).
// - label_accumulate: per-center sum/count scatter for the Lloyd update.
//
// MFMA notes (gfx950): v_mfma_f32_32x32x2_f32 — exact f32 at the 157 TF
// vector rate; lane l supplies A[i=l&31][k=l>>5] and B[k=l>>5][j=l&31];
// C/D element (reg, lane) -> row=(reg&3)+8*(reg>>2)+4*(lane>>5), col=lane&31.
// Wave = 64 lanes. The 128-wide dot tiles (kmeans_assign, dbscan_sweep, gram) stage BK=64
// k-major LDS tiles padded to a 129-float row stride so the transposing
// staging writes spread over the banks; the 32-lane MFMA operand reads are
// unit-stride along a row.

#include <torch/extension.h>
#include <c10/hip/HIPException.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

using f32x16 = __attribute__((ext_vector_type(16))) float;

// ---------------------------------------------------------------------------
// kmeans_assign: fused X·C^T (MFMA) + ||x||²+||c||²−2x·c + running argmin.
//
// Grid: one block per 128-row slice of X. Each block loops over all center
// tiles (BN=128) and, per tile, over d in BK=64 steps with LDS-staged X and C
// tiles. 4 waves, each computing a 2x2 grid of 32x32 MFMA tiles. The per-row
// running (dist,center) is kept packed in a 64-bit LDS word (float-bits<<32 |
// center) updated with atomicMin — float bits of non-negative distances sort
// correctly as unsigned.
// ---------------------------------------------------------------------------

constexpr int KM_BM = 128;
constexpr int KM_BN = 128;
constexpr int KM_BK = 64;
constexpr int KM_LD = KM_BK * KM_BM / 256;  // staging elems per thread (32)

__global__ __launch_bounds__(256) void kmeans_assign_kernel(
    const float* __restrict__ X,     // [n,d] row-major
    const float* __restrict__ C,     // [k,d] row-major
    const float* __restrict__ x_sq,  // [n]
    const float* __restrict__ c_sq,  // [k]
    int n, int d, int k,
    int32_t* __restrict__ labels,    // [n]
    float* __restrict__ min_dists,   // [n] squared distance to the winner
    double* __restrict__ inertia) {  // [1] accumulated
  // Single-buffer BK=64 with write-after-barrier register pipelining (T14):
  // per K-step 128 MFMAs (8192 issue cycles/wave) run between two barriers;
  // the next tile's registers are written right after the first barrier and
  // the tile after that's global loads are issued immediately, so HBM
  // latency hides under the MFMA phase. As compiled (ROCm 7.2 clang, -O3):
  // 256 VGPR + 256 AGPR with spills, 67 KB LDS -> 1 wave/SIMD, one block/CU.
  __shared__ float lds_x[KM_BK][KM_BM + 1];
  __shared__ float lds_c[KM_BK][KM_BN + 1];
  __shared__ unsigned long long best[KM_BM];

  const int i0 = blockIdx.x * KM_BM;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wr = wave >> 1;  // wave row (0..1) -> 64 rows
  const int wc = wave & 1;   // wave col (0..1) -> 64 cols

  for (int i = tid; i < KM_BM; i += blockDim.x) best[i] = ~0ULL;

  const bool full_rows = (i0 + KM_BM <= n);
  const int nsteps = (d + KM_BK - 1) / KM_BK;
  float rx[KM_LD], rc[KM_LD];

  for (int j0 = 0; j0 < k; j0 += KM_BN) {
    const bool full_cols = (j0 + KM_BN <= k);
    f32x16 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int nn = 0; nn < 2; ++nn)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][nn][r] = 0.0f;

    // loads: KM_LD=32 elems/thread; e = q*256+tid over 8192 = 128 rows x 64 kd
#define KM_LOAD_T(dst, SRC, base_row, d0)                                      \
  do {                                                                         \
    if (full_rows && full_cols && (d0) + KM_BK <= d) {                         \
      _Pragma("unroll") for (int q = 0; q < KM_LD; ++q) {                      \
        int e = q * 256 + tid;                                                 \
        dst[q] = SRC[(int64_t)((base_row) + (e >> 6)) * d + (d0) + (e & 63)];  \
      }                                                                        \
    } else {                                                                   \
      _Pragma("unroll") for (int q = 0; q < KM_LD; ++q) {                      \
        int e = q * 256 + tid;                                                 \
        int gr = (base_row) + (e >> 6);                                        \
        int gd = (d0) + (e & 63);                                              \
        int lim = (&dst[0] == &rx[0]) ? n : k;                                 \
        dst[q] = (gr < lim && gd < d) ? SRC[(int64_t)gr * d + gd] : 0.0f;      \
      }                                                                        \
    }                                                                          \
  } while (0)

#define KM_WRITE()                                                             \
  do {                                                                         \
    _Pragma("unroll") for (int q = 0; q < KM_LD; ++q) {                        \
      int e = q * 256 + tid;                                                   \
      lds_x[e & 63][e >> 6] = rx[q];                                           \
      lds_c[e & 63][e >> 6] = rc[q];                                           \
    }                                                                          \
  } while (0)

    // prologue: tile 0 into LDS, tile 1 into regs
    KM_LOAD_T(rx, X, i0, 0);
    KM_LOAD_T(rc, C, j0, 0);
    __syncthreads();  // best[] init / previous epilogue complete
    KM_WRITE();
    if (nsteps > 1) {
      KM_LOAD_T(rx, X, i0, KM_BK);
      KM_LOAD_T(rc, C, j0, KM_BK);
    }
    __syncthreads();

    for (int step = 0; step < nsteps; ++step) {
#pragma unroll 8
      for (int kk = 0; kk < KM_BK / 2; ++kk) {
        const int kd = 2 * kk + (lane >> 5);
        float a0 = lds_x[kd][wr * 64 + (lane & 31)];
        float a1 = lds_x[kd][wr * 64 + 32 + (lane & 31)];
        float b0 = lds_c[kd][wc * 64 + (lane & 31)];
        float b1 = lds_c[kd][wc * 64 + 32 + (lane & 31)];
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
      }
      __syncthreads();  // all waves done reading this tile
      if (step + 1 < nsteps) {
        KM_WRITE();  // vmcnt-waits for loads issued a full MFMA phase ago
        if (step + 2 < nsteps) {
          KM_LOAD_T(rx, X, i0, (step + 2) * KM_BK);
          KM_LOAD_T(rc, C, j0, (step + 2) * KM_BK);
        }
        __syncthreads();
      }
    }
#undef KM_LOAD_T
#undef KM_WRITE

    // epilogue: distances + packed argmin into LDS
#pragma unroll
    for (int m = 0; m < 2; ++m) {
#pragma unroll
      for (int nn = 0; nn < 2; ++nn) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          int row = wr * 64 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
          int col = wc * 64 + nn * 32 + (lane & 31);
          int gi = i0 + row, gj = j0 + col;
          if (gi < n && gj < k) {
            float dist = x_sq[gi] + c_sq[gj] - 2.0f * acc[m][nn][r];
            dist = dist < 0.0f ? 0.0f : dist;
            unsigned long long packed =
                ((unsigned long long)__float_as_uint(dist) << 32) |
                (unsigned int)gj;
            atomicMin(&best[row], packed);
          }
        }
      }
    }
    __syncthreads();
  }

  // write labels / min dists; block-reduce inertia
  __shared__ double block_inertia[4];
  double partial = 0.0;
  for (int i = tid; i < KM_BM; i += blockDim.x) {
    int gi = i0 + i;
    if (gi < n) {
      unsigned long long p = best[i];
      float dist = __uint_as_float((unsigned int)(p >> 32));
      labels[gi] = (int32_t)(p & 0xffffffffu);
      min_dists[gi] = dist;
      partial += (double)dist;
    }
  }
  // wave reduce
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    partial += __shfl_down(partial, off, 64);
  if (lane == 0) block_inertia[wave] = partial;
  __syncthreads();
  if (tid == 0) {
    double s = block_inertia[0] + block_inertia[1] + block_inertia[2] + block_inertia[3];
    atomicAdd(inertia, s);
  }
}





// ---------------------------------------------------------------------------
// dbscan_sweep: fused n x n eps-neighborhood pass for DBSCAN, reusing the
// kmeans_assign tile structure (rows = this rank's slice of the replicated
// dataset, "centers" = ALL rows, tiled by 128). The torch path materializes
// [chunk, n] masked int64 label tensors (~8 bytes x n per row per sweep of
// pure HBM traffic); here the distance never leaves registers and the
// epilogue reduces straight into a 128-entry LDS accumulator.
//   mode 0: out[i] = #{ j : d2(i,j) <= eps2 }            (core counting)
//   mode 1: out[i] = min{ labels[j] : core[j], d2 <= eps2 }  (label sweep /
//           border assignment; 0x7fffffff when no core neighbor)
// One kernel serves core detection, the min-label propagation sweeps and
// the border pass (reference DBSCANMG: adjacency + BFS inside cuML,
// SURVEY.md §2.3b).
//
// Ball-cover pruning (reference algorithm="rbc", clustering.py:686-695):
// when tile_off != nullptr the column loop walks only the CSR list of
// admissible 128-column tiles for this 128-row block — tiles whose bounding
// ball can contain an eps-neighbor of the row block's ball (triangle
// inequality, computed host-side after a coarse-kmeans row permutation).
// The per-pair eps test below is unchanged, so results are exact.
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(256) void dbscan_sweep_kernel(
    const float* __restrict__ X,       // [n,d] replicated rows
    const float* __restrict__ x_sq,    // [n]
    int n, int d,
    int row0, int n_rows,              // this rank's slice [row0, row0+n_rows)
    float eps2, int mode,
    const uint8_t* __restrict__ core,  // [n] (mode 1)
    const int32_t* __restrict__ labels,// [n] (mode 1)
    const int32_t* __restrict__ tile_idx, // CSR col-tile ids (nullptr = dense)
    const int32_t* __restrict__ tile_off, // [n_row_blocks+1] (nullptr = dense)
    int32_t* __restrict__ out) {       // [n_rows]
  __shared__ float lds_x[KM_BK][KM_BM + 1];
  __shared__ float lds_c[KM_BK][KM_BN + 1];
  __shared__ int acc_row[KM_BM];

  const int i0 = row0 + blockIdx.x * KM_BM;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wr = wave >> 1;
  const int wc = wave & 1;
  const int row_lim = row0 + n_rows;

  for (int i = tid; i < KM_BM; i += blockDim.x)
    acc_row[i] = (mode == 0) ? 0 : 0x7fffffff;

  const bool full_rows = (i0 + KM_BM <= row_lim);
  const int nsteps = (d + KM_BK - 1) / KM_BK;
  float rx[KM_LD], rc[KM_LD];
  // per-lane per-fragment-row accumulator carried across ALL column tiles:
  // dense data fires an LDS atomic per in-eps PAIR otherwise (~5e10 atomics
  // on 20-blob 1M x 64 — the label sweep cost 2.6x the count pass)
  int racc[2][16];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) racc[m][r] = (mode == 0) ? 0 : 0x7fffffff;

  const bool pruned = (tile_off != nullptr);
  const int t_beg = pruned ? tile_off[blockIdx.x] : 0;
  const int t_end = pruned ? tile_off[blockIdx.x + 1] : (n + KM_BN - 1) / KM_BN;
  for (int t = t_beg; t < t_end; ++t) {
    const int j0 = (pruned ? tile_idx[t] : t) * KM_BN;
    const bool full_cols = (j0 + KM_BN <= n);
    f32x16 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int nn = 0; nn < 2; ++nn)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][nn][r] = 0.0f;

#define DB_LOAD_T(dst, base_row, lim, d0)                                      \
  do {                                                                         \
    if (full_rows && full_cols && (d0) + KM_BK <= d) {                         \
      _Pragma("unroll") for (int q = 0; q < KM_LD; ++q) {                      \
        int e = q * 256 + tid;                                                 \
        dst[q] = X[(int64_t)((base_row) + (e >> 6)) * d + (d0) + (e & 63)];    \
      }                                                                        \
    } else {                                                                   \
      _Pragma("unroll") for (int q = 0; q < KM_LD; ++q) {                      \
        int e = q * 256 + tid;                                                 \
        int gr = (base_row) + (e >> 6);                                        \
        int gd = (d0) + (e & 63);                                              \
        dst[q] = (gr < (lim) && gd < d) ? X[(int64_t)gr * d + gd] : 0.0f;      \
      }                                                                        \
    }                                                                          \
  } while (0)

#define DB_WRITE()                                                             \
  do {                                                                         \
    _Pragma("unroll") for (int q = 0; q < KM_LD; ++q) {                        \
      int e = q * 256 + tid;                                                   \
      lds_x[e & 63][e >> 6] = rx[q];                                           \
      lds_c[e & 63][e >> 6] = rc[q];                                           \
    }                                                                          \
  } while (0)

    DB_LOAD_T(rx, i0, row_lim, 0);
    DB_LOAD_T(rc, j0, n, 0);
    __syncthreads();
    DB_WRITE();
    if (nsteps > 1) {
      DB_LOAD_T(rx, i0, row_lim, KM_BK);
      DB_LOAD_T(rc, j0, n, KM_BK);
    }
    __syncthreads();

    for (int step = 0; step < nsteps; ++step) {
#pragma unroll 8
      for (int kk = 0; kk < KM_BK / 2; ++kk) {
        const int kd = 2 * kk + (lane >> 5);
        float a0 = lds_x[kd][wr * 64 + (lane & 31)];
        float a1 = lds_x[kd][wr * 64 + 32 + (lane & 31)];
        float b0 = lds_c[kd][wc * 64 + (lane & 31)];
        float b1 = lds_c[kd][wc * 64 + 32 + (lane & 31)];
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
      }
      __syncthreads();
      if (step + 1 < nsteps) {
        DB_WRITE();
        if (step + 2 < nsteps) {
          DB_LOAD_T(rx, i0, row_lim, (step + 2) * KM_BK);
          DB_LOAD_T(rc, j0, n, (step + 2) * KM_BK);
        }
        __syncthreads();
      }
    }
#undef DB_LOAD_T
#undef DB_WRITE

    // epilogue: per-lane only 2 distinct columns -> hoist the per-column
    // gathers (x_sq / core / labels) out of the 32-row loop
#pragma unroll
    for (int nn = 0; nn < 2; ++nn) {
      const int col = wc * 64 + nn * 32 + (lane & 31);
      const int gj = j0 + col;
      if (gj >= n) continue;
      const float cs = x_sq[gj];
      int lab_j = 0;
      bool core_j = true;
      if (mode == 1) {
        core_j = core[gj] != 0;
        if (core_j) lab_j = labels[gj];
      }
      if (mode == 1 && !core_j) continue;
#pragma unroll
      for (int m = 0; m < 2; ++m) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          int row = wr * 64 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
          int gi = i0 + row;
          if (gi < row_lim) {
            float d2 = x_sq[gi] + cs - 2.0f * acc[m][nn][r];
            if (d2 <= eps2) {
              if (mode == 0)
                ++racc[m][r];
              else
                racc[m][r] = min(racc[m][r], lab_j);
            }
          }
        }
      }
    }
    __syncthreads();
  }

  // one LDS atomic per fragment row for the whole kernel
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      int row = wr * 64 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      if (mode == 0) {
        if (racc[m][r]) atomicAdd(&acc_row[row], racc[m][r]);
      } else if (racc[m][r] != 0x7fffffff) {
        atomicMin(&acc_row[row], racc[m][r]);
      }
    }
  __syncthreads();

  for (int i = tid; i < KM_BM; i += blockDim.x) {
    int gi = i0 + i;
    if (gi < row_lim) out[gi - row0] = acc_row[i];
  }
}


// ---------------------------------------------------------------------------
// UMAP edge-sampled SGD (reference: cuML UMAP optimize_layout,
// SURVEY.md §2.3b umap fit). One thread per edge per epoch, Hogwild
// atomicAdd updates (the torch path's index_add is the same semantics with
// ~10 kernel launches + intermediate tensors per epoch; here one launch per
// epoch and the epoch loop lives in the host wrapper). Negative samples use
// a per-(edge, epoch, trial) wang-hash — distributionally equivalent to the
// torch generator, not bit-identical (UMAP is stochastic either way).
// ---------------------------------------------------------------------------

__device__ __forceinline__ unsigned umap_hash(unsigned x) {
  x = (x ^ 61u) ^ (x >> 16);
  x *= 9u;
  x = x ^ (x >> 4);
  x *= 0x27d4eb2du;
  x = x ^ (x >> 15);
  return x;
}

template <int DIM>
__global__ __launch_bounds__(256) void umap_sgd_epoch_kernel(
    float* __restrict__ emb,            // [n_head, DIM] updated in place
    float* __restrict__ tail_emb,       // [n_vertices, DIM] (== emb when fitting)
    const int32_t* __restrict__ heads,  // [m]
    const int32_t* __restrict__ tails,  // [m]
    const float* __restrict__ eps,      // [m] epochs-per-sample
    float* __restrict__ next_due,       // [m] state
    int m, int n_vertices,
    float a, float b, float alpha, float repulsion,
    int neg_rate, int move_tail, int epoch, unsigned seed) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  if (next_due[i] > (float)epoch) return;
  next_due[i] += eps[i];

  const float clip = 4.0f;
  const int h = heads[i], t = tails[i];
  // head update accumulates in REGISTERS across the positive edge and all
  // negative samples (sequential-local semantics, like umap-learn's CPU
  // loop), committed with ONE atomic per component at the end — the
  // per-sample version fired 2+2*neg_rate head atomics per due edge and the
  // atomic pipe (not bandwidth) bounded the epoch.
  float eh[DIM], diff[DIM], upd[DIM];
  float d2 = 0.0f;
#pragma unroll
  for (int c = 0; c < DIM; ++c) {
    eh[c] = emb[(int64_t)h * DIM + c];
    upd[c] = 0.0f;
    diff[c] = eh[c] - tail_emb[(int64_t)t * DIM + c];
    d2 += diff[c] * diff[c];
  }
  float d2c = fmaxf(d2, 1e-12f);
  float pb = __powf(d2c, b);
  float gcoef = (-2.0f * a * b * pb / d2c) / (1.0f + a * pb);
#pragma unroll
  for (int c = 0; c < DIM; ++c) {
    float g = fminf(fmaxf(gcoef * diff[c], -clip), clip);
    upd[c] += g;
    if (move_tail) atomicAdd(&tail_emb[(int64_t)t * DIM + c], -alpha * g);
  }

  unsigned rng = umap_hash(seed ^ umap_hash((unsigned)i * 2654435761u + (unsigned)epoch));
  for (int r = 0; r < neg_rate; ++r) {
    rng = umap_hash(rng + 0x9e3779b9u + (unsigned)r);
    int j = (int)(rng % (unsigned)n_vertices);
    d2 = 0.0f;
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      diff[c] = (eh[c] + alpha * upd[c]) - tail_emb[(int64_t)j * DIM + c];
      d2 += diff[c] * diff[c];
    }
    d2c = fmaxf(d2, 1e-12f);
    pb = __powf(d2c, b);
    gcoef = (2.0f * repulsion * b) / ((0.001f + d2) * (1.0f + a * pb));
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      float g = fminf(fmaxf(gcoef * diff[c], -clip), clip);
      upd[c] += g;
    }
  }
#pragma unroll
  for (int c = 0; c < DIM; ++c)
    if (upd[c] != 0.0f) atomicAdd(&emb[(int64_t)h * DIM + c], alpha * upd[c]);
}

// ---------------------------------------------------------------------------
// label_accumulate: sums[label[i]] += X[i], counts[label[i]] += 1 via a
// sort-based segmented reduction: rows pre-sorted by label (torch.sort in
// the wrapper), each (label, split) block register-accumulates its column
// stripe over its row sub-segment — each X element is read ONCE, coalesced,
// and the only atomics are the k*SPLIT partial merges.
// ---------------------------------------------------------------------------

constexpr int LA_SPLIT = 8;    // sub-segments per label (skew tolerance)
constexpr int LA_COLS = 16;    // column accumulators per thread (256*16=4096)

__global__ __launch_bounds__(256) void segment_sum_kernel(
    const float* __restrict__ X, const int64_t* __restrict__ perm,
    const int64_t* __restrict__ seg_off, int d,
    float* __restrict__ sums, float* __restrict__ counts) {
  const int lab = blockIdx.x / LA_SPLIT;
  const int split = blockIdx.x % LA_SPLIT;
  const int64_t s0 = seg_off[lab], e0 = seg_off[lab + 1];
  const int64_t len = e0 - s0;
  if (len == 0) return;
  const int64_t chunk = (len + LA_SPLIT - 1) / LA_SPLIT;
  const int64_t rs = s0 + split * chunk;
  const int64_t re = min(e0, rs + chunk);
  if (rs >= re) return;
  if (split == 0 && threadIdx.x == 0) counts[lab] = (float)len;

  for (int cb = 0; cb < d; cb += blockDim.x * LA_COLS) {
    float acc[LA_COLS];
#pragma unroll
    for (int q = 0; q < LA_COLS; ++q) acc[q] = 0.0f;
    int64_t r = rs;
    for (; r + 4 <= re; r += 4) {  // 4 rows in flight for latency hiding
      const float* row0 = X + perm[r] * (int64_t)d;
      const float* row1 = X + perm[r + 1] * (int64_t)d;
      const float* row2 = X + perm[r + 2] * (int64_t)d;
      const float* row3 = X + perm[r + 3] * (int64_t)d;
#pragma unroll
      for (int q = 0; q < LA_COLS; ++q) {
        int c = cb + q * blockDim.x + threadIdx.x;
        if (c < d) acc[q] += row0[c] + row1[c] + row2[c] + row3[c];
      }
    }
    for (; r < re; ++r) {
      const float* row = X + perm[r] * (int64_t)d;
#pragma unroll
      for (int q = 0; q < LA_COLS; ++q) {
        int c = cb + q * blockDim.x + threadIdx.x;
        if (c < d) acc[q] += row[c];
      }
    }
#pragma unroll
    for (int q = 0; q < LA_COLS; ++q) {
      int c = cb + q * blockDim.x + threadIdx.x;
      if (c < d) {
        if (LA_SPLIT > 1)
          atomicAdd(&sums[(int64_t)lab * d + c], acc[q]);
        else
          sums[(int64_t)lab * d + c] = acc[q];
      }
    }
  }
}

// ---------------------------------------------------------------------------
// segment_sum_inertia: segment_sum that also returns sum_i |x_i - c_label(i)|^2.
// A block streams the rows of ONE label over its column stripe, so it keeps
// that centre's stripe in registers and squares (x - c) beside the sum: no
// further pass over X. The squares are summed in f32 over one 4-row group of
// the thread's columns (64 terms), then added into a double; one f64 atomic
// per block. The direct difference has no |x|^2 + |c|^2 - 2x.c cancellation.
// Per column the rows are added in segment_sum's order and grouping, so sums
// and counts equal label_accumulate's. VEC (d % 4 == 0, 16-byte aligned
// bases): each lane loads float4s, 4 per row instead of 16 scalars.
// ---------------------------------------------------------------------------

constexpr bool LA_VEC_DEFAULT = true;

template <bool VEC>
__global__ __launch_bounds__(256) void segment_sum_inertia_kernel(
    const float* __restrict__ X, const int64_t* __restrict__ perm,
    const int64_t* __restrict__ seg_off, const float* __restrict__ C, int d,
    float* __restrict__ sums, float* __restrict__ counts,
    double* __restrict__ inertia) {
  constexpr int W = VEC ? 4 : 1;      // columns per load
  constexpr int NQ = LA_COLS / W;     // loads per thread and row
  const int lab = blockIdx.x / LA_SPLIT;
  const int split = blockIdx.x % LA_SPLIT;
  const int64_t s0 = seg_off[lab], e0 = seg_off[lab + 1];
  const int64_t len = e0 - s0;
  if (len == 0) return;
  const int64_t chunk = (len + LA_SPLIT - 1) / LA_SPLIT;
  const int64_t rs = s0 + split * chunk;
  const int64_t re = min(e0, rs + chunk);
  if (rs >= re) return;  // block-uniform: no barrier is skipped by part of a block
  if (split == 0 && threadIdx.x == 0) counts[lab] = (float)len;

  auto ld = [](const float* p, float* out) {
    if constexpr (VEC) {
      const float4 v = *reinterpret_cast<const float4*>(p);
      out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
    } else {
      out[0] = *p;
    }
  };

  const float* crow = C + (int64_t)lab * d;
  double local = 0.0;
  for (int cb = 0; cb < d; cb += blockDim.x * LA_COLS) {
    float acc[LA_COLS], cen[LA_COLS];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int c = cb + (q * blockDim.x + threadIdx.x) * W;
#pragma unroll
      for (int w = 0; w < W; ++w) { acc[q * W + w] = 0.0f; cen[q * W + w] = 0.0f; }
      if (c < d) ld(crow + c, cen + q * W);  // VEC: d % 4 == 0, all 4 inside
    }
    int64_t r = rs;
    for (; r + 4 <= re; r += 4) {  // 4 rows in flight for latency hiding
      const float* row0 = X + perm[r] * (int64_t)d;
      const float* row1 = X + perm[r + 1] * (int64_t)d;
      const float* row2 = X + perm[r + 2] * (int64_t)d;
      const float* row3 = X + perm[r + 3] * (int64_t)d;
      float part = 0.0f;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int c = cb + (q * blockDim.x + threadIdx.x) * W;
        if (c < d) {
          float x0[W], x1[W], x2[W], x3[W];
          ld(row0 + c, x0); ld(row1 + c, x1); ld(row2 + c, x2); ld(row3 + c, x3);
#pragma unroll
          for (int w = 0; w < W; ++w) {
            const float ce = cen[q * W + w];
            acc[q * W + w] += x0[w] + x1[w] + x2[w] + x3[w];
            const float f0 = x0[w] - ce, f1 = x1[w] - ce, f2 = x2[w] - ce, f3 = x3[w] - ce;
            part = fmaf(f0, f0, part); part = fmaf(f1, f1, part);
            part = fmaf(f2, f2, part); part = fmaf(f3, f3, part);
          }
        }
      }
      local += (double)part;
    }
    for (; r < re; ++r) {
      const float* row = X + perm[r] * (int64_t)d;
      float part = 0.0f;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int c = cb + (q * blockDim.x + threadIdx.x) * W;
        if (c < d) {
          float x0[W];
          ld(row + c, x0);
#pragma unroll
          for (int w = 0; w < W; ++w) {
            acc[q * W + w] += x0[w];
            const float f0 = x0[w] - cen[q * W + w];
            part = fmaf(f0, f0, part);
          }
        }
      }
      local += (double)part;
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int c = cb + (q * blockDim.x + threadIdx.x) * W;
      if (c < d) {
#pragma unroll
        for (int w = 0; w < W; ++w) {
          if (LA_SPLIT > 1)
            atomicAdd(&sums[(int64_t)lab * d + c + w], acc[q * W + w]);
          else
            sums[(int64_t)lab * d + c + w] = acc[q * W + w];
        }
      }
    }
  }
  __shared__ double red_s[256];
  red_s[threadIdx.x] = local;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (threadIdx.x < off) red_s[threadIdx.x] += red_s[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) atomicAdd(inertia, red_s[0]);
}

// ---------------------------------------------------------------------------
// label_accumulate_lds: direct one-pass scatter for small k*d. Each block
// owns an LDS-private [k,d] f32 accumulator (+ k counts), streams its row
// range in NATURAL order — X read once, coalesced, no sort and no permuted
// gather — and atomically merges into global once at the end (same
// privatization pattern as csr_grad). Used when k*d*4 <= 120 KB: on the
// BASELINE k=200 d=128 config the sort+segment path's permuted row gather
// ran at ~0.4 TB/s (128 ms for 51 GB); this pass is a plain streaming read.
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(512) void label_accumulate_lds_kernel(
    const float* __restrict__ X, const int32_t* __restrict__ labels,
    int64_t n, int d, int k, int64_t rows_per_block,
    float* __restrict__ sums, float* __restrict__ counts) {
  extern __shared__ float lacc[];  // [k*d] sums then [k] counts
  float* lcnt = lacc + (size_t)k * d;
  const int kd = k * d;
  for (int i = threadIdx.x; i < kd + k; i += blockDim.x) lacc[i] = 0.0f;
  __syncthreads();
  const int64_t rs = (int64_t)blockIdx.x * rows_per_block;
  const int64_t re = min(n, rs + rows_per_block);
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int nw = (int)(blockDim.x >> 6);
  if ((d & 1) == 0 && d <= 128) {
    // float2 row reads (d=128 -> one 512 B wave access covers the row).
    // Two-deep software pipeline over 8-row groups: the ISA of the naive
    // form showed 8 SERIALIZED uniform label loads (staggered vmcnt(7..0))
    // and no cross-iteration overlap — ~2 full HBM latencies per group per
    // wave. Here the 8 labels arrive in ONE 8-lane load (broadcast by
    // shuffles) and the NEXT group's label+row loads are issued before the
    // current group's waits, so every address (a function of r alone)
    // pipelines.
    const int d2i = d >> 1;
    const bool act = lane < d2i;
    // each wave streams a CONTIGUOUS row slice: an 8-row group is one 4 KB
    // burst (the interleaved wave-stride layout issued 8 scattered 512 B
    // segments per group and capped at ~790 GB/s)
    const int64_t span = (re - rs + nw - 1) / nw;
    int64_t r = min(re, rs + (int64_t)wave * span);
    const int64_t we = min(re, r + span);
    int labv = (lane < 8 && r + lane < we) ? labels[r + lane] : 0;
    float2 va[8], vb[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int64_t rr = r + q;
      va[q] = (act && rr < we)
                  ? reinterpret_cast<const float2*>(X + rr * (int64_t)d)[lane]
                  : float2{0.0f, 0.0f};
    }
    for (; r + 7 < we;) {
      const int64_t rn = r + 8;
      int labn = 0;
      if (rn + 7 < we) {
        labn = (lane < 8) ? labels[rn + lane] : 0;
#pragma unroll
        for (int q = 0; q < 8; ++q)
          vb[q] = act ? reinterpret_cast<const float2*>(
                            X + (rn + q) * (int64_t)d)[lane]
                      : float2{0.0f, 0.0f};
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int lq = __shfl(labv, q, 64);
        float* dst = lacc + (size_t)lq * d;
        if (act) {
          atomicAdd(&dst[2 * lane], va[q].x);
          atomicAdd(&dst[2 * lane + 1], va[q].y);
        }
        if (lane == 0) atomicAdd(&lcnt[lq], 1.0f);
      }
      r = rn;
      labv = labn;
#pragma unroll
      for (int q = 0; q < 8; ++q) va[q] = vb[q];
    }
    for (; r < we; ++r) {
      const float2* row = reinterpret_cast<const float2*>(X + r * (int64_t)d);
      float* dst = lacc + (size_t)labels[r] * d;
      for (int c2 = lane; c2 < d2i; c2 += 64) {
        float2 v = row[c2];
        atomicAdd(&dst[2 * c2], v.x);
        atomicAdd(&dst[2 * c2 + 1], v.y);
      }
      if (lane == 0) atomicAdd(&lcnt[labels[r]], 1.0f);
    }
  } else if ((d & 1) == 0) {
    int64_t r = rs + wave;
    for (; r < re; r += nw) {
      const float2* row = reinterpret_cast<const float2*>(X + r * (int64_t)d);
      float* dst = lacc + (size_t)labels[r] * d;
      for (int c2 = lane; c2 < (d >> 1); c2 += 64) {
        float2 v = row[c2];
        atomicAdd(&dst[2 * c2], v.x);
        atomicAdd(&dst[2 * c2 + 1], v.y);
      }
      if (lane == 0) atomicAdd(&lcnt[labels[r]], 1.0f);
    }
  } else {
    for (int64_t r = rs + wave; r < re; r += nw) {
      const float* row = X + r * (int64_t)d;
      float* dst = lacc + (size_t)labels[r] * d;
      for (int c = lane; c < d; c += 64) atomicAdd(&dst[c], row[c]);
      if (lane == 0) atomicAdd(&lcnt[labels[r]], 1.0f);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kd; i += blockDim.x)
    if (lacc[i] != 0.0f) atomicAdd(&sums[i], lacc[i]);
  for (int i = threadIdx.x; i < k; i += blockDim.x)
    if (lcnt[i] != 0.0f) atomicAdd(&counts[i], lcnt[i]);
}

// ---------------------------------------------------------------------------
// gram_f32: C[d,d] = A^T A for A [n,d] row-major (TN MFMA GEMM).
// Upper blocks only would halve work; full matrix kept for simplicity —
// the symmetric skip is a planned optimization.
// ---------------------------------------------------------------------------

constexpr int GR_BM = 128;
constexpr int GR_BN = 128;
constexpr int GR_BK = 64;
constexpr int GR_LD = GR_BK * GR_BM / 256;  // 32 staging elems per thread

// gram_kernel: C[d,d] = A^T A, upper-triangle block enumeration (1D grid of
// nb*(nb+1)/2 tiles x SPLIT row-slices; partials atomicAdd'ed) with the
// same BK=64 write-after-barrier pipeline as the kmeans assign kernel.
__global__ __launch_bounds__(256) void gram_kernel(
    const float* __restrict__ A, int64_t n, int d, int nb, int split,
    float* __restrict__ out) {
  __shared__ float lds_i[GR_BK][GR_BM + 1];
  __shared__ float lds_j[GR_BK][GR_BN + 1];

  const int tri = blockIdx.x / split;
  const int slice = blockIdx.x % split;
  // tri -> (bi, bj) upper triangle: bi = row of the triangle
  int bi = (int)((sqrtf(8.0f * tri + 1.0f) - 1.0f) * 0.5f);
  while ((bi + 1) * (bi + 2) / 2 <= tri) ++bi;
  while (bi * (bi + 1) / 2 > tri) --bi;
  const int bj_off = tri - bi * (bi + 1) / 2;
  const int j0 = bi * GR_BN;          // bi-th diagonal stripe
  const int i0 = bj_off * GR_BM;      // column tile within the stripe (i0<=j0)

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wr = wave >> 1;
  const int wc = wave & 1;

  const int nsteps_total = (int)((n + GR_BK - 1) / GR_BK);
  const int per = (nsteps_total + split - 1) / split;
  const int s_begin = slice * per;
  const int s_end = min(nsteps_total, s_begin + per);
  if (s_begin >= s_end) return;

  const bool full_i = (i0 + GR_BM <= d);
  const bool full_j = (j0 + GR_BN <= d);

  f32x16 acc[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int nn = 0; nn < 2; ++nn)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][nn][r] = 0.0f;

  float rg[GR_LD];

#define GR_LOAD(dst_unused, col0, step, full)                                  \
  do {                                                                         \
    int64_t r0 = (int64_t)(step)*GR_BK;                                        \
    if ((full) && r0 + GR_BK <= n) {                                           \
      _Pragma("unroll") for (int q = 0; q < GR_LD; ++q) {                      \
        int e = q * 256 + tid;                                                 \
        rg[q] = A[(r0 + (e >> 7)) * d + (col0) + (e & 127)];                   \
      }                                                                        \
    } else {                                                                   \
      _Pragma("unroll") for (int q = 0; q < GR_LD; ++q) {                      \
        int e = q * 256 + tid;                                                 \
        int64_t gr = r0 + (e >> 7);                                            \
        int gc = (col0) + (e & 127);                                           \
        rg[q] = (gr < n && gc < d) ? A[gr * d + gc] : 0.0f;                    \
      }                                                                        \
    }                                                                          \
  } while (0)

#define GR_WRITE(dstlds)                                                       \
  do {                                                                         \
    _Pragma("unroll") for (int q = 0; q < GR_LD; ++q) {                        \
      int e = q * 256 + tid;                                                   \
      dstlds[e >> 7][e & 127] = rg[q];                                         \
    }                                                                          \
  } while (0)

  // Staging: consecutive lanes take consecutive COLUMNS of one data row
  // (row-major A -> coalesced 512B reads); LDS write [rr][i] is contiguous.
  GR_LOAD(rg, i0, s_begin, full_i);
  GR_WRITE(lds_i);
  GR_LOAD(rg, j0, s_begin, full_j);
  GR_WRITE(lds_j);
  __syncthreads();

  for (int step = s_begin; step < s_end; ++step) {
#pragma unroll 8
    for (int kk = 0; kk < GR_BK / 2; ++kk) {
      const int rr = 2 * kk + (lane >> 5);
      float a0 = lds_i[rr][wr * 64 + (lane & 31)];
      float a1 = lds_i[rr][wr * 64 + 32 + (lane & 31)];
      float b0 = lds_j[rr][wc * 64 + (lane & 31)];
      float b1 = lds_j[rr][wc * 64 + 32 + (lane & 31)];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();
    if (step + 1 < s_end) {
      GR_LOAD(rg, i0, step + 1, full_i);
      GR_WRITE(lds_i);
      GR_LOAD(rg, j0, step + 1, full_j);
      GR_WRITE(lds_j);
      __syncthreads();
    }
  }
#undef GR_LOAD
#undef GR_WRITE

#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int nn = 0; nn < 2; ++nn)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        int row = i0 + wr * 64 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        int col = j0 + wc * 64 + nn * 32 + (lane & 31);
        if (row < d && col < d && col >= row) {
          float v = acc[m][nn][r];
          if (split > 1) {
            atomicAdd(&out[(int64_t)row * d + col], v);
          } else {
            out[(int64_t)row * d + col] = v;
          }
        }
      }
}

// mirror upper triangle to lower
__global__ void gram_mirror_kernel(float* __restrict__ out, int d) {
  int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t total = (int64_t)d * d;
  for (; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    int row = (int)(idx / d), col = (int)(idx % d);
    if (col < row) out[idx] = out[(int64_t)col * d + row];
  }
}

// ---------------------------------------------------------------------------
// knn_select: fused brute-force k-NN — MFMA distance tiles + in-LDS
// per-query top-k (reference NearestNeighborsMG's tiled ||x-y||^2 + top-k
// merge, SURVEY.md §2.3b knn.py:763-774). No [nq, ni] distance matrix is
// materialized: each 64-query block streams item tiles, keeps an unsorted
// k-candidate pool per query in LDS (one merge lane per query, current-max
// cached in registers), and writes its item-range partial top-k; partials
// across item splits merge on the host side (torch.topk over [q, S*k]).
// k <= 64.
// ---------------------------------------------------------------------------

constexpr int KN_QB = 64;    // queries per block
constexpr int KN_IB = 128;   // items per tile
constexpr int KN_BK = 32;    // d chunk
constexpr int KN_KMAX = 64;

__global__ __launch_bounds__(256) void knn_select_kernel(
    const float* __restrict__ Q,     // [nq, d]
    const float* __restrict__ I,     // [ni, d]
    const float* __restrict__ q_sq,  // [nq]
    const float* __restrict__ i_sq,  // [ni]
    int nq, int ni, int d, int k, int isplit,
    float* __restrict__ out_dist,    // [nq, isplit, k]
    int32_t* __restrict__ out_idx) { // [nq, isplit, k]
  // floats: lds_q [32][65], lds_i [32][129], dist [64][129], pool u64[64][k]
  __shared__ __attribute__((aligned(16))) float smem[32 * 65 + 32 * 129 + 64 * 129 +
                                                     2 * KN_QB * KN_KMAX];
  constexpr int SQ = 0;
  constexpr int SI = 32 * 65;
  constexpr int SD = SI + 32 * 129;
  constexpr int SP = SD + 64 * 129;

  const int q0 = (blockIdx.x / isplit) * KN_QB;
  const int split = blockIdx.x % isplit;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wr = wave >> 1;  // 0..1 query half (32 rows)
  const int wc = wave & 1;   // 0..1 item half (64 cols)

  unsigned long long* pool = reinterpret_cast<unsigned long long*>(&smem[SP]);
  for (int e = tid; e < KN_QB * k; e += 256) pool[e] = ~0ULL;

  const int per = (ni + isplit - 1) / isplit;
  const int it_begin = split * per;
  const int it_end = min(ni, it_begin + per);

  // merge-lane registers: thread t (<64) owns query q0+t
  float cur_max = __uint_as_float(0x7f7fffffu);  // FLT_MAX
  int cur_pos = 0;
  int filled = 0;

  for (int ib = it_begin; ib < it_end; ib += KN_IB) {
    f32x16 acc[2];
#pragma unroll
    for (int nn = 0; nn < 2; ++nn)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[nn][r] = 0.0f;

    const bool tile_full = (q0 + KN_QB <= nq) && (ib + KN_IB <= it_end);
    for (int d0 = 0; d0 < d; d0 += KN_BK) {
      // stage Q[q0:q0+64, d0:+32] -> lds_q[kd][row], I tile likewise.
      // Guards hoisted to tile level (per-element selects de-pipeline
      // hipcc, guide §5.4 trap (c)).
      if (tile_full && d0 + KN_BK <= d) {
#pragma unroll 4
        for (int e = tid; e < KN_QB * KN_BK; e += 256) {
          int row = e >> 5, kd = e & 31;
          smem[SQ + kd * 65 + row] = Q[(int64_t)(q0 + row) * d + d0 + kd];
        }
#pragma unroll 4
        for (int e = tid; e < KN_IB * KN_BK; e += 256) {
          int row = e >> 5, kd = e & 31;
          smem[SI + kd * 129 + row] = I[(int64_t)(ib + row) * d + d0 + kd];
        }
      } else {
        for (int e = tid; e < KN_QB * KN_BK; e += 256) {
          int row = e >> 5, kd = e & 31;
          int gq = q0 + row, gd = d0 + kd;
          smem[SQ + kd * 65 + row] =
              (gq < nq && gd < d) ? Q[(int64_t)gq * d + gd] : 0.0f;
        }
        for (int e = tid; e < KN_IB * KN_BK; e += 256) {
          int row = e >> 5, kd = e & 31;
          int gi = ib + row, gd = d0 + kd;
          smem[SI + kd * 129 + row] =
              (gi < it_end && gd < d) ? I[(int64_t)gi * d + gd] : 0.0f;
        }
      }
      __syncthreads();
#pragma unroll 8
      for (int kk = 0; kk < KN_BK / 2; ++kk) {
        const int kd = 2 * kk + (lane >> 5);
        float a = smem[SQ + kd * 65 + wr * 32 + (lane & 31)];
        float b0 = smem[SI + kd * 129 + wc * 64 + (lane & 31)];
        float b1 = smem[SI + kd * 129 + wc * 64 + 32 + (lane & 31)];
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc[1], 0, 0, 0);
      }
      __syncthreads();
    }

    // distances into SD[row][col]
#pragma unroll
    for (int nn = 0; nn < 2; ++nn) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        int row = wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        int col = wc * 64 + nn * 32 + (lane & 31);
        int gq = q0 + row, gi = ib + col;
        float dist = 3.4e38f;
        if (gq < nq && gi < it_end) {
          dist = q_sq[gq] + i_sq[gi] - 2.0f * acc[nn][r];
          dist = dist < 0.0f ? 0.0f : dist;
        }
        smem[SD + row * 129 + col] = dist;
      }
    }
    __syncthreads();

    // merge: lane t of waves 0-? — threads 0..63 each own one query row
    if (tid < KN_QB) {
      const int q = tid;
      unsigned long long* mypool = pool + q * k;
      const int lim = min(KN_IB, it_end - ib);
      for (int j = 0; j < lim; ++j) {
        float dd = smem[SD + q * 129 + j];
        if (filled < k) {
          mypool[filled] =
              ((unsigned long long)__float_as_uint(dd) << 32) | (unsigned)(ib + j);
          ++filled;
          if (filled == k) {  // establish current max
            cur_max = -1.0f;
            for (int t2 = 0; t2 < k; ++t2) {
              float v = __uint_as_float((unsigned)(mypool[t2] >> 32));
              if (v > cur_max) { cur_max = v; cur_pos = t2; }
            }
          }
        } else if (dd < cur_max) {
          mypool[cur_pos] =
              ((unsigned long long)__float_as_uint(dd) << 32) | (unsigned)(ib + j);
          cur_max = -1.0f;
          for (int t2 = 0; t2 < k; ++t2) {  // rescan for new max
            float v = __uint_as_float((unsigned)(mypool[t2] >> 32));
            if (v > cur_max) { cur_max = v; cur_pos = t2; }
          }
        }
      }
    }
    __syncthreads();
  }

  // write partials (sorted ascending by simple selection — k<=64)
  if (tid < KN_QB) {
    const int q = tid;
    if (q0 + q < nq) {
      unsigned long long* mypool = pool + q * k;
      for (int a = 0; a < k; ++a) {  // selection sort in LDS
        int best_t = a;
        unsigned long long bv = mypool[a];
        for (int b = a + 1; b < k; ++b)
          if (mypool[b] < bv) { bv = mypool[b]; best_t = b; }
        unsigned long long tmp = mypool[a];
        mypool[a] = bv;
        mypool[best_t] = tmp;
        bool invalid = (bv & 0xffffffffu) == 0xffffffffu;
        float dv = invalid ? 3.4e38f : __uint_as_float((unsigned)(bv >> 32));
        int64_t off = ((int64_t)(q0 + q) * isplit + split) * k + a;
        out_dist[off] = dv;
        out_idx[off] = invalid ? -1 : (int32_t)(bv & 0xffffffffu);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// rf_histogram: per-(node, feature, bin[, class]) histograms for random
// forest split finding (reference: cuML RF histogram build, SURVEY.md §2.3b
// tree.py:384-389). Rows pre-sorted by node (perm + seg_off, as in
// segment_sum); each (node, row-split) block accumulates its feature-chunk
// histogram in LDS (fast LDS atomics) and adds it to global once.
// Classification: C channels of class counts. Regression (n_classes==0):
// 2 channels (count, sum) — sum-of-squares cancels in the gain.
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(256) void rf_histogram_kernel(
    const uint8_t* __restrict__ Xcm,  // [d, n_phys] binned, COLUMN-major:
                                      // per-feature columns keep a segment's
                                      // row gathers inside dense cache lines
                                      // (row-major fetched ~47 64B lines per
                                      // row to use 54 sampled bytes)
    const int64_t* __restrict__ perm, // [m] VIRTUAL rows sorted by node
    const int64_t* __restrict__ seg_off,  // [B+1]
    const int32_t* __restrict__ feat_sel, // [B, mf] or nullptr (identity)
    const int32_t* __restrict__ y_cls,    // [n_phys] class ids (classification)
    const float* __restrict__ y_reg,      // [n_phys] targets (regression)
    const int32_t* __restrict__ sample,   // [vn] virtual->physical, or nullptr
    int64_t n_phys,                       // modulo map when sample==nullptr
    int d, int mf, int f0, int FC, int n_bins, int C, int split,
    float y_inv_scale,                    // regression: 1/max|y| for the
                                          // packed-u64 path; 0 = disabled
    float y_scale,                        //             max|y|
    float* __restrict__ out) {            // [B, FC, n_bins, C]
  // lhist [FC][nb][C] + an LDS copy of the block's feature-id chunk; the
  // hot loop gathers FOUR feature bytes per row before touching LDS so the
  // dependent L2/HBM gather latencies overlap (the naive one-at-a-time loop
  // ran ~12 cycles/update, far off the LDS-atomic bound)
  extern __shared__ __attribute__((aligned(16))) float lhist[];
  // per-feature COLUMN BASE OFFSETS (f * n_phys precomputed once — the
  // per-element int64 multiply cost ~3 issue slots in the hot loop);
  // region rounded up to 8B alignment (odd nfc with odd bins*classes)
  int64_t* foff_s =
      reinterpret_cast<int64_t*>(lhist + ((FC * n_bins * C + 1) & ~1));
  const int b = blockIdx.x / split;
  const int slice = blockIdx.x % split;
  const int64_t s0 = seg_off[b], e0 = seg_off[b + 1];
  const int64_t len = e0 - s0;
  const int tid = threadIdx.x;
  const int nfc = FC * n_bins * C;
  if (len == 0) {
    // split==1 gets an UNINITIALIZED out buffer (no host zero-fill): an
    // empty segment must still define its cells
    if (split == 1) {
      float* dst0 = out + (int64_t)b * nfc;
      for (int e = tid; e < nfc; e += 256) dst0[e] = 0.0f;
    }
    return;
  }
  const int64_t chunk = (len + split - 1) / split;
  const int64_t rs = s0 + slice * chunk;
  const int64_t re = min(e0, rs + chunk);
  if (rs >= re) return;
  for (int e = tid; e < nfc; e += 256) lhist[e] = 0.0f;
  for (int e = tid; e < FC; e += 256) {
    const int f = feat_sel ? feat_sel[(int64_t)b * mf + f0 + e] : (f0 + e);
    foff_s[e] = (int64_t)f * n_phys;
  }
  __syncthreads();

  const bool classif = (y_cls != nullptr);
  for (int64_t r = rs + tid; r < re; r += 256) {
    const int64_t vrow = perm[r];
    const int64_t row = sample ? (int64_t)sample[vrow]
                               : (vrow >= n_phys ? vrow % n_phys : vrow);
    const int yc = classif ? y_cls[row] : 0;
    const float yv = classif ? 1.0f : y_reg[row];
    // regression fast path: ONE u64 LDS atomic per (row, feature) — count
    // in bits 41+, biased Q14 fixed-point sum of y/max|y| below (each
    // contribution positive, so carries never cross the field boundary;
    // count <= 2^23 rows per node enforced host-side)
    const bool packed = !classif && y_inv_scale > 0.0f;
    unsigned long long yq = 0;
    if (packed) {
      const long long fix = llroundf(yv * y_inv_scale * 16384.0f) + (1ll << 15);
      yq = (1ull << 41) + (unsigned long long)fix;
    }
    int q = 0;
    for (; q + 7 < FC; q += 8) {
      int bins[8];
#pragma unroll
      for (int e = 0; e < 8; ++e)
        bins[e] = Xcm[foff_s[q + e] + row];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if (classif) {
          atomicAdd(&lhist[((q + e) * n_bins + bins[e]) * C + yc], 1.0f);
        } else if (packed) {
          atomicAdd(reinterpret_cast<unsigned long long*>(lhist) +
                        (q + e) * n_bins + bins[e],
                    yq);
        } else {
          float* cell = &lhist[((q + e) * n_bins + bins[e]) * 2];
          atomicAdd(cell, 1.0f);
          atomicAdd(cell + 1, yv);
        }
      }
    }
    for (; q < FC; ++q) {
      const int bin = Xcm[foff_s[q] + row];
      if (classif) {
        atomicAdd(&lhist[(q * n_bins + bin) * C + yc], 1.0f);
      } else if (packed) {
        atomicAdd(reinterpret_cast<unsigned long long*>(lhist) + q * n_bins + bin,
                  yq);
      } else {
        float* cell = &lhist[(q * n_bins + bin) * 2];
        atomicAdd(cell, 1.0f);
        atomicAdd(cell + 1, yv);
      }
    }
  }
  __syncthreads();

  float* dst = out + (int64_t)b * FC * n_bins * C;
  const bool packed_flush = (y_cls == nullptr) && y_inv_scale > 0.0f;
  if (!packed_flush) {
    if (split > 1) {
      for (int e = tid; e < nfc; e += 256)
        if (lhist[e] != 0.0f) atomicAdd(&dst[e], lhist[e]);
    } else {
      for (int e = tid; e < nfc; e += 256) dst[e] = lhist[e];
    }
  } else {
    // decode packed (count, biased Q14 sum) -> the [.., 2] float layout
    const unsigned long long* ph =
        reinterpret_cast<const unsigned long long*>(lhist);
    for (int e2 = tid; e2 < FC * n_bins; e2 += 256) {
      const unsigned long long v = ph[e2];
      const long long cnt = (long long)(v >> 41);
      const long long sq =
          (long long)(v & ((1ull << 41) - 1)) - cnt * (1ll << 15);
      const float sum = (float)sq * (y_scale / 16384.0f);
      if (split > 1) {
        if (cnt) {
          atomicAdd(&dst[e2 * 2], (float)cnt);
          atomicAdd(&dst[e2 * 2 + 1], sum);
        }
      } else {
        dst[e2 * 2] = (float)cnt;
        dst[e2 * 2 + 1] = sum;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// rf_histogram_fw: feature-wide variant — LANES run over (sorted) sampled
// features of ONE row, the loop runs over rows. The row-lane kernel above
// issued one address-divergent gather per (row, feature): each wave-load
// touched up to 64 distinct cache lines and the LSU serialized them
// (~28 cyc/update, invariant under unrolls/LDS/atomic-count experiments).
// Here a wave-load reads 32 SORTED features of one row — a short span of
// the row-major row (avg gap d/mf) — so the per-update issue cost drops by
// the lane width. Two rows per wave (lane groups of 32). Regression uses
// the packed single-u64-atomic cells.
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(256) void rf_histogram_fw_kernel(
    const uint8_t* __restrict__ Xrm,  // [n_phys, d] ROW-major
    const int64_t* __restrict__ perm,
    const int64_t* __restrict__ seg_off,  // [B+1]
    const int32_t* __restrict__ feat_sel, // [B, mf] SORTED per node, or null
    const int32_t* __restrict__ y_cls,
    const float* __restrict__ y_reg,
    const int32_t* __restrict__ sample,
    int64_t n_phys,
    int d, int mf, int f0, int FC, int n_bins, int C, int split,
    float y_inv_scale, float y_scale,
    float* __restrict__ out) {            // [B, FC, n_bins, C]
  extern __shared__ __attribute__((aligned(16))) float lhist[];
  int* fsel_s = reinterpret_cast<int*>(
      lhist + (((int64_t)FC * n_bins * C + 1) & ~1ll));
  const int b = blockIdx.x / split;
  const int slice = blockIdx.x % split;
  const int64_t s0 = seg_off[b], e0 = seg_off[b + 1];
  const int64_t len = e0 - s0;
  const int tid = threadIdx.x;
  const int nfc = FC * n_bins * C;
  const bool classif = (y_cls != nullptr);
  const bool packed = !classif && y_inv_scale > 0.0f;
  if (len == 0) {
    if (split == 1) {
      float* dst0 = out + (int64_t)b * nfc;
      for (int e = tid; e < nfc; e += 256) dst0[e] = 0.0f;
    }
    return;
  }
  const int64_t chunk = (len + split - 1) / split;
  const int64_t rs = s0 + slice * chunk;
  const int64_t re = min(e0, rs + chunk);
  if (rs >= re) return;

  for (int e = tid; e < nfc; e += 256) lhist[e] = 0.0f;
  for (int e = tid; e < FC; e += 256)
    fsel_s[e] = feat_sel ? feat_sel[(int64_t)b * mf + f0 + e] : (f0 + e);
  __syncthreads();

  // 32 rows per block iteration: 8 lane-groups x 4 INDEPENDENT row chains
  // per group — the perm->sample->row->gather dependency is ~3 serial
  // memory latencies; one chain per group left waves issue-stalled (PMC:
  // 71% SQ_WAIT_INST_ANY), four chains quadruple the loads in flight
  const int group = tid >> 5;       // 0..7
  const int fq = tid & 31;          // feature slot within the chunk
  const int f = (fq < FC) ? fsel_s[fq] : -1;
  for (int64_t base = rs; base < re; base += 32) {
    int64_t rowv[4];
    int binv[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int64_t r = base + group + 8 * g;
      if (r < re) {
        const int64_t vrow = perm[r];
        rowv[g] = sample ? (int64_t)sample[vrow]
                         : (vrow >= n_phys ? vrow % n_phys : vrow);
      } else {
        rowv[g] = -1;
      }
    }
#pragma unroll
    for (int g = 0; g < 4; ++g)
      binv[g] = (rowv[g] >= 0 && f >= 0) ? Xrm[rowv[g] * d + f] : -1;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      if (binv[g] < 0) continue;
      const int64_t row = rowv[g];
      const int bin = binv[g];
      if (classif) {
        atomicAdd(&lhist[(fq * n_bins + bin) * C + y_cls[row]], 1.0f);
      } else if (packed) {
        const long long fix =
            llroundf(y_reg[row] * y_inv_scale * 16384.0f) + (1ll << 15);
        atomicAdd(reinterpret_cast<unsigned long long*>(lhist) + fq * n_bins + bin,
                  (1ull << 41) + (unsigned long long)fix);
      } else {
        float* cell = &lhist[(fq * n_bins + bin) * 2];
        atomicAdd(cell, 1.0f);
        atomicAdd(cell + 1, y_reg[row]);
      }
    }
  }
  __syncthreads();

  float* dst = out + (int64_t)b * nfc;
  if (!packed) {
    if (split > 1) {
      for (int e = tid; e < nfc; e += 256)
        if (lhist[e] != 0.0f) atomicAdd(&dst[e], lhist[e]);
    } else {
      for (int e = tid; e < nfc; e += 256) dst[e] = lhist[e];
    }
  } else {
    const unsigned long long* ph =
        reinterpret_cast<const unsigned long long*>(lhist);
    for (int e2 = tid; e2 < FC * n_bins; e2 += 256) {
      const unsigned long long v = ph[e2];
      const long long cnt = (long long)(v >> 41);
      const long long sq =
          (long long)(v & ((1ull << 41) - 1)) - cnt * (1ll << 15);
      const float sum = (float)sq * (y_scale / 16384.0f);
      if (split > 1) {
        if (cnt) {
          atomicAdd(&dst[e2 * 2], (float)cnt);
          atomicAdd(&dst[e2 * 2 + 1], sum);
        }
      } else {
        dst[e2 * 2] = (float)cnt;
        dst[e2 * 2 + 1] = sum;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// rf_best_split: fused split-finding scan over rf_histogram output.
// One block per node: threads own features, scan bins accumulating left
// stats in registers, compute the gain (gini for classification; the
// cancelled-sum-of-squares form for regression), block-reduce the best
// (gain, feature, bin) and emit the winning child stats. Replaces the
// torch cumsum/where/max/gather chain (~25% of RF fit).
// C (=classes, or 2 regression channels) <= 16.
// ---------------------------------------------------------------------------

constexpr int RS_CMAX = 16;

__global__ __launch_bounds__(256) void rf_best_split_kernel(
    const float* __restrict__ H,  // [B, F, nb, C]
    int F, int nb, int C, int min_leaf, int classif,
    float* __restrict__ out_gain,   // [B]
    int32_t* __restrict__ out_feat, // [B] (chunk-local feature idx)
    int32_t* __restrict__ out_bin,  // [B]
    float* __restrict__ out_lval,   // [B, C]
    float* __restrict__ out_rval) { // [B, C]
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const float* Hb = H + (int64_t)b * F * nb * C;

  float best_gain = -1.0f;
  int best_f = -1, best_bin = -1;

  for (int f = tid; f < F; f += 256) {
    const float* Hf = Hb + (int64_t)f * nb * C;
    float total[RS_CMAX];
    for (int c = 0; c < C; ++c) total[c] = 0.0f;
    for (int bin = 0; bin < nb; ++bin)
      for (int c = 0; c < C; ++c) total[c] += Hf[bin * C + c];
    float tcnt = 0.0f, tsum = 0.0f, tsq = 0.0f;
    if (classif) {
      for (int c = 0; c < C; ++c) {
        tcnt += total[c];
        tsq += total[c] * total[c];
      }
    } else {
      tcnt = total[0];
      tsum = total[1];
    }
    if (tcnt < 2 * min_leaf) continue;

    float left[RS_CMAX];
    for (int c = 0; c < C; ++c) left[c] = 0.0f;
    float lcnt = 0.0f, lsum = 0.0f, lsq = 0.0f;
    for (int bin = 0; bin < nb - 1; ++bin) {
      if (classif) {
        for (int c = 0; c < C; ++c) {
          float v = Hf[bin * C + c];
          lsq += v * (2.0f * left[c] + v);  // maintain sum of left[c]^2
          left[c] += v;
          lcnt += v;
        }
        float rcnt = tcnt - lcnt;
        if (lcnt >= min_leaf && rcnt >= min_leaf) {
          // gini gain = g_parent - (l/t) g_l - (r/t) g_r
          float rsq = 0.0f;
          for (int c = 0; c < C; ++c) {
            float rv = total[c] - left[c];
            rsq += rv * rv;
          }
          float g_p = 1.0f - tsq / (tcnt * tcnt);
          float g_l = 1.0f - lsq / (lcnt * lcnt);
          float g_r = 1.0f - rsq / (rcnt * rcnt);
          float gain = g_p - (lcnt / tcnt) * g_l - (rcnt / tcnt) * g_r;
          if (gain > best_gain) { best_gain = gain; best_f = f; best_bin = bin; }
        }
      } else {
        lcnt += Hf[bin * C + 0];
        lsum += Hf[bin * C + 1];
        float rcnt = tcnt - lcnt, rsum = tsum - lsum;
        if (lcnt >= min_leaf && rcnt >= min_leaf) {
          float gain = (lsum * lsum / lcnt + rsum * rsum / rcnt -
                        tsum * tsum / tcnt) / tcnt;
          if (gain > best_gain) { best_gain = gain; best_f = f; best_bin = bin; }
        }
      }
    }
  }

  // block-reduce best (gain, f, bin): pack gain bits (non-negative or -1)
  __shared__ unsigned long long red[4];
  unsigned long long mine =
      ((unsigned long long)__float_as_uint(best_gain + 2.0f) << 32) |
      ((unsigned)(best_f & 0xffff) << 16) | (unsigned)(best_bin & 0xffff);
  // wave max
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    unsigned long long o = __shfl_down(mine, off, 64);
    if (o > mine) mine = o;
  }
  if ((tid & 63) == 0) red[tid >> 6] = mine;
  __syncthreads();
  if (tid == 0) {
    unsigned long long m = red[0];
    for (int w = 1; w < 4; ++w)
      if (red[w] > m) m = red[w];
    float g = __uint_as_float((unsigned)(m >> 32)) - 2.0f;
    int f = (int)((m >> 16) & 0xffff);
    int bin = (int)(m & 0xffff);
    if (f == 0xffff) { f = -1; }
    if (bin == 0xffff) { bin = -1; }
    out_gain[b] = g;
    out_feat[b] = f;
    out_bin[b] = bin;
    if (f >= 0 && bin >= 0) {
      const float* Hf = Hb + (int64_t)f * nb * C;
      for (int c = 0; c < C; ++c) {
        float l = 0.0f, t = 0.0f;
        for (int bb = 0; bb <= bin; ++bb) l += Hf[bb * C + c];
        for (int bb = 0; bb < nb; ++bb) t += Hf[bb * C + c];
        out_lval[(int64_t)b * C + c] = l;
        out_rval[(int64_t)b * C + c] = t - l;
      }
    } else {
      for (int c = 0; c < C; ++c) {
        out_lval[(int64_t)b * C + c] = 0.0f;
        out_rval[(int64_t)b * C + c] = 0.0f;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// kmeans_argmin_kn: fused epilogue over a library-GEMM dot block.
// dots is [k, n] (C @ X^T): per row i the k dot values sit at stride n, so
// the 256 threads of a block read coalesced spans per center. d2 =
// c_sq[kk] - 2*dot (x_sq[i] added once at the end). One pass over the
// [k, n] block; c_sq staged in LDS. The all-in-one MFMA assign kernel runs
// at 84 TF; hipBLASLt runs the same dot block at 141 TF, so GEMM + this
// bandwidth-bound pass wins (measured; SRML_KMEANS_VARIANT=fused keeps the
// old path).
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(256) void kmeans_argmin_kn_kernel(
    const float* __restrict__ dots,  // [k, n]
    const float* __restrict__ x_sq,  // [n]
    const float* __restrict__ c_sq,  // [k]
    int64_t n, int k,
    int32_t* __restrict__ labels,    // [n]
    float* __restrict__ min_d,       // [n] squared distance to winner
    double* __restrict__ inertia) {  // [1] accumulated
  extern __shared__ float csq_s[];
  for (int e = threadIdx.x; e < k; e += 256) csq_s[e] = c_sq[e];
  __syncthreads();
  double local_sum = 0.0;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    float best = 3.0e38f;
    int bi = 0;
    for (int kk = 0; kk < k; ++kk) {
      const float v = csq_s[kk] - 2.0f * dots[(int64_t)kk * n + i];
      if (v < best) { best = v; bi = kk; }
    }
    const float d2 = fmaxf(best + x_sq[i], 0.0f);
    labels[i] = bi;
    min_d[i] = d2;
    local_sum += (double)d2;
  }
  // block-reduce the inertia partial, one global atomic per block
  __shared__ double red_s[256];
  red_s[threadIdx.x] = local_sum;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (threadIdx.x < off) red_s[threadIdx.x] += red_s[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) atomicAdd(inertia, red_s[0]);
}

// ---------------------------------------------------------------------------
// kmeans_argmin_nk: argmin epilogue over a ROW-major [m, k] dot block
// (dots = X_chunk @ C^T — the tall-skinny GEMM hipBLASLt runs at full rate,
// unlike the [k, n] layout whose skinny-m GEMM stalls at small k). One wave
// per row: lanes stride k contiguously (coalesced), then a shuffle
// argmin-reduce; block accumulates inertia with one atomic.
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(256) void kmeans_argmin_nk_kernel(
    const float* __restrict__ dots,  // [m, k] row-major
    const float* __restrict__ x_sq,  // [m]
    const float* __restrict__ c_sq,  // [k]
    int64_t m, int k,
    int32_t* __restrict__ labels,    // [m]
    float* __restrict__ min_d,       // [m]
    double* __restrict__ inertia) {  // [1]
  __shared__ double block_in[4];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  // grid-stride over rows: the grid is capped (<=4096 blocks) so the
  // inertia merge is one atomic per BLOCK, not per row — a block-per-row
  // launch serializes millions of f64 atomics on one word
  const int64_t wstride = (int64_t)gridDim.x * 4;
  double local = 0.0;
  for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < m; row += wstride) {
    const float* dr = dots + row * (int64_t)k;
    float best = 3.0e38f;
    int bj = 0;
    for (int j = lane; j < k; j += 64) {
      const float v = c_sq[j] - 2.0f * dr[j];
      if (v < best) { best = v; bj = j; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ob = __shfl_down(best, off, 64);
      const int oj = __shfl_down(bj, off, 64);
      if (ob < best) { best = ob; bj = oj; }
    }
    if (lane == 0) {
      const float d2 = fmaxf(best + x_sq[row], 0.0f);
      labels[row] = bj;
      min_d[row] = d2;
      local += (double)d2;
    }
  }
  if (lane == 0) block_in[wave] = local;
  __syncthreads();
  if (threadIdx.x == 0)
    atomicAdd(inertia, block_in[0] + block_in[1] + block_in[2] + block_in[3]);
}

// ---------------------------------------------------------------------------
// Split-bf16 screened assignment (ops/kmeans.py `_assign_split`).
// The f32 GEMM of the "kn" path is bound by the f32 MFMA rate; the argmin
// only needs dots good enough to separate the best two centres. Every value
// is centred (x' = x - mu, mu = column mean of C: distances are translation
// invariant) and split into bf16 hi + lo; the library bf16 GEMM (f32 out,
// f32 accumulate) forms hi*hi + hi*lo + lo*hi, whose error is
// <= 3*2^-18 |x'||c'| (u = 2^-9: |x - hi - lo| <= u^2|x|, the dropped lo*lo
// and the two residuals are each <= u^2 sum|x_i c_i|). Rows whose best two
// screened values lie within 4*eps*|x'|*max|c'| (eps = 2^-15) are decided in
// double from the original data; every other row's screen argmin is exact.
//
// kmeans_split_bf16: one wave per row. S row = [hi(0..d) | 0 | lo(0..d) | 0],
// each half dp = ceil32(d) wide, so both halves start 16-byte aligned.
// Lanes walk groups of 8 columns: two 16-byte loads, one 16-byte store per
// half; VEC=false (d % 4 != 0: rows are not 16-byte aligned) loads scalars.
// LO=false (kmeans_split_bf16_hi) neither computes nor stores the lo half:
// S row = [hi(0..d) | 0], dp wide, same hi bits and same a_sq.
// ---------------------------------------------------------------------------

__device__ __forceinline__ uint32_t bf16_rne_bits(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

template <bool VEC, bool LO>
__global__ __launch_bounds__(256) void kmeans_split_bf16_kernel(
    const float* __restrict__ A,    // [m, d]
    const float* __restrict__ mu,   // [d]
    int64_t m, int d, int dp,
    uint16_t* __restrict__ S,       // [m, 2*dp] bf16 bits; [m, dp] without LO
    float* __restrict__ a_sq) {     // [m]
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int groups = dp >> 3;
  const int64_t wstride = (int64_t)gridDim.x * 4;
  for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < m; row += wstride) {
    const float* ar = A + row * (int64_t)d;
    uint16_t* sr = S + row * (int64_t)(LO ? 2 * dp : dp);
    float acc = 0.0f;
    for (int g = lane; g < groups; g += 64) {
      const int c0 = g * 8;
      float x[8];
      if (VEC) {
        // d % 4 == 0: a float4 is either wholly inside the row or wholly pad
        float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0;
        if (c0 < d) {
          const float4 a0 = *reinterpret_cast<const float4*>(ar + c0);
          const float4 m0 = *reinterpret_cast<const float4*>(mu + c0);
          v0 = make_float4(a0.x - m0.x, a0.y - m0.y, a0.z - m0.z, a0.w - m0.w);
        }
        if (c0 + 4 < d) {
          const float4 a1 = *reinterpret_cast<const float4*>(ar + c0 + 4);
          const float4 m1 = *reinterpret_cast<const float4*>(mu + c0 + 4);
          v1 = make_float4(a1.x - m1.x, a1.y - m1.y, a1.z - m1.z, a1.w - m1.w);
        }
        x[0] = v0.x; x[1] = v0.y; x[2] = v0.z; x[3] = v0.w;
        x[4] = v1.x; x[5] = v1.y; x[6] = v1.z; x[7] = v1.w;
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e)
          x[e] = (c0 + e < d) ? ar[c0 + e] - mu[c0 + e] : 0.0f;
      }
      uint32_t hb[8], lb[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        hb[e] = bf16_rne_bits(x[e]);
        // x - hi is exact in f32 (hi carries the top 8 significand bits)
        if (LO) lb[e] = bf16_rne_bits(x[e] - __uint_as_float(hb[e] << 16));
        acc = fmaf(x[e], x[e], acc);
      }
      uint4 ho;
      ho.x = hb[0] | (hb[1] << 16); ho.y = hb[2] | (hb[3] << 16);
      ho.z = hb[4] | (hb[5] << 16); ho.w = hb[6] | (hb[7] << 16);
      *reinterpret_cast<uint4*>(sr + c0) = ho;
      if (LO) {
        uint4 lo;
        lo.x = lb[0] | (lb[1] << 16); lo.y = lb[2] | (lb[3] << 16);
        lo.z = lb[4] | (lb[5] << 16); lo.w = lb[6] | (lb[7] << 16);
        *reinterpret_cast<uint4*>(sr + dp + c0) = lo;
      }
    }
    double s = (double)acc;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if (lane == 0) a_sq[row] = (float)s;
  }
}

// ---------------------------------------------------------------------------
// kmeans_argmin_kn_screen: kmeans_argmin_kn's loop over the screened [k, m]
// dot block, keeping best and second-best v = c_sq - 2*dot. A row whose
// second is within margin_scale*sqrt(a_sq) of its best is appended to
// flagged_rows (one atomic per wave) and left for kmeans_refine; every other
// row is final here. One thread per row; the loop over centres is batched
// and branch-free so the loads of a batch are in flight together: 5.7 TB/s on
// the 4 GB block of 1M rows x k=1000, against 2.4 TB/s for one dependent
// compare-and-branch per load (profiles/README.md "Prepared X").
// ---------------------------------------------------------------------------

constexpr int SCREEN_BATCH = 8;  // centres loaded per row before any is used

__global__ __launch_bounds__(256) void kmeans_argmin_kn_screen_kernel(
    const float* __restrict__ dots,   // [k, m]
    const float* __restrict__ a_sq,   // [m] centred |x'|^2
    const float* __restrict__ c_sq,   // [k] centred |c'|^2
    const float* __restrict__ margin_scale,  // [1] 4*eps*max_j|c'_j|
    int64_t m, int k,
    int32_t* __restrict__ labels,     // [m]
    float* __restrict__ min_d,        // [m]
    double* __restrict__ inertia,     // [1] accumulated
    int32_t* __restrict__ flagged_rows,  // [m]
    int32_t* __restrict__ n_flagged) {   // [1] accumulated
  extern __shared__ float csq_s[];
  for (int e = threadIdx.x; e < k; e += 256) csq_s[e] = c_sq[e];
  __syncthreads();
  const float ms = margin_scale[0];
  const int lane = threadIdx.x & 63;
  double local_sum = 0.0;
  const int64_t stride = (int64_t)gridDim.x * 256;
  // i0 is block-uniform so every lane reaches the ballot below
  for (int64_t i0 = (int64_t)blockIdx.x * 256; i0 < m; i0 += stride) {
    const int64_t i = i0 + threadIdx.x;
    const bool valid = i < m;
    float best = 3.0e38f, second = 3.0e38f;
    int bi = 0;
    if (valid) {
      // SCREEN_BATCH independent loads are issued before the first is used,
      // and the update is select-only: v < best shifts best into second,
      // otherwise second = min(second, v) (an equal v keeps the lower index
      // and lands in second, as the branchy form did).
      const float* col = dots + i;
      int kk = 0;
      for (; kk + SCREEN_BATCH <= k; kk += SCREEN_BATCH) {
        float dv[SCREEN_BATCH];
#pragma unroll
        for (int u = 0; u < SCREEN_BATCH; ++u) dv[u] = col[(int64_t)(kk + u) * m];
#pragma unroll
        for (int u = 0; u < SCREEN_BATCH; ++u) {
          const float v = csq_s[kk + u] - 2.0f * dv[u];
          const bool lt = v < best;
          second = lt ? best : fminf(second, v);
          bi = lt ? kk + u : bi;
          best = lt ? v : best;
        }
      }
      for (; kk < k; ++kk) {
        const float v = csq_s[kk] - 2.0f * col[(int64_t)kk * m];
        const bool lt = v < best;
        second = lt ? best : fminf(second, v);
        bi = lt ? kk : bi;
        best = lt ? v : best;
      }
    }
    const float asq = valid ? a_sq[i] : 0.0f;
    const bool flag = valid && second <= best + ms * sqrtf(asq);
    if (valid && !flag) {
      const float d2 = fmaxf(best + asq, 0.0f);
      labels[i] = bi;
      min_d[i] = d2;
      local_sum += (double)d2;
    }
    const unsigned long long mask = __ballot(flag);
    if (mask != 0ull) {
      const int leader = __ffsll((long long)mask) - 1;
      int base = 0;
      if (lane == leader) base = atomicAdd(n_flagged, __popcll(mask));
      base = __shfl(base, leader, 64);
      if (flag)
        flagged_rows[base + __popcll(mask & ((1ull << lane) - 1ull))] = (int32_t)i;
    }
  }
  __shared__ double red_s[256];
  red_s[threadIdx.x] = local_sum;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (threadIdx.x < off) red_s[threadIdx.x] += red_s[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) atomicAdd(inertia, red_s[0]);
}

// ---------------------------------------------------------------------------
// kmeans_refine: one wave per flagged row, grid-stride over the device-side
// list. Rescans the row's k screened values for its best, then decides among
// every centre within the margin by sum((double)x - (double)c)^2 over the
// ORIGINAL (uncentred) data; candidates are visited in ascending index and
// replaced only on strictly smaller, so the lowest index wins a tie.
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(256) void kmeans_refine_kernel(
    const float* __restrict__ X,      // [m, d] original rows of this chunk
    const float* __restrict__ C,      // [k, d] original centres
    const float* __restrict__ dots,   // [k, m] screened
    const float* __restrict__ c_sq,   // [k] centred
    const float* __restrict__ a_sq,   // [m] centred
    const float* __restrict__ margin_scale,  // [1]
    const int32_t* __restrict__ flagged_rows,
    const int32_t* __restrict__ n_flagged,
    int64_t m, int d, int k,
    int32_t* __restrict__ labels, float* __restrict__ min_d,
    double* __restrict__ inertia) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int64_t nf = min((int64_t)n_flagged[0], m);
  const float ms = margin_scale[0];
  const int64_t wstride = (int64_t)gridDim.x * 4;
  double local = 0.0;
  for (int64_t f = (int64_t)blockIdx.x * 4 + wave; f < nf; f += wstride) {
    const int64_t r = flagged_rows[f];
    float best = 3.0e38f;
    for (int j = lane; j < k; j += 64)
      best = fminf(best, c_sq[j] - 2.0f * dots[(int64_t)j * m + r]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) best = fminf(best, __shfl_xor(best, off, 64));
    const float thr = best + ms * sqrtf(a_sq[r]);
    const float* xr = X + r * (int64_t)d;
    double bd = 1.0e300;
    int bj = 0;
    // j0 is wave-uniform so the ballot sees all 64 lanes
    for (int j0 = 0; j0 < k; j0 += 64) {
      const int j = j0 + lane;
      const bool cand = j < k && (c_sq[j] - 2.0f * dots[(int64_t)j * m + r]) <= thr;
      unsigned long long mask = __ballot(cand);
      while (mask != 0ull) {
        const int b = __ffsll((long long)mask) - 1;
        mask &= mask - 1ull;
        const float* cr = C + (int64_t)(j0 + b) * d;
        double s = 0.0;
        for (int e = lane; e < d; e += 64) {
          const double df = (double)xr[e] - (double)cr[e];
          s = fma(df, df, s);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
        if (s < bd) { bd = s; bj = j0 + b; }
      }
    }
    if (lane == 0) {
      labels[r] = bj;
      min_d[r] = (float)bd;
      local += bd;
    }
  }
  if (lane == 0 && local != 0.0) atomicAdd(inertia, local);
}

// ---------------------------------------------------------------------------
// rf_partition: counting-sort rows by batch-local node id -> (perm, seg_off).
// Replaces the per-batch torch sort + nonzero + gather chain (radix sort was
// ~8% of RF fit kernel time; reference behavior: cuML's batched node trainer
// keeps per-node row lists, tree.py:384-389).
// Two kernels: block-privatized LDS count, then a two-pass scatter where each
// block reserves per-node ranges with ONE global atomic per (block, node)
// and places its rows via LDS-local cursors (a single global cursor per node
// would serialize ~n atomics on one word at depth 0).
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(256) void rf_node_count_kernel(
    const int64_t* __restrict__ node_of_row,  // [n]
    const int64_t* __restrict__ lut,          // [n_nodes] node -> slot | -1
    int64_t n, int B,
    int32_t* __restrict__ counts) {           // [B] pre-zeroed
  extern __shared__ int32_t lcnt0[];
  for (int e = threadIdx.x; e < B; e += 256) lcnt0[e] = 0;
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const int64_t sl = lut[node_of_row[i]];
    if (sl >= 0) atomicAdd(&lcnt0[sl], 1);
  }
  __syncthreads();
  for (int e = threadIdx.x; e < B; e += 256)
    if (lcnt0[e]) atomicAdd(&counts[e], lcnt0[e]);
}

__global__ __launch_bounds__(256) void rf_partition_scatter_kernel(
    const int64_t* __restrict__ node_of_row,  // [n]
    const int64_t* __restrict__ lut,          // node -> slot | -1
    int64_t n, int B,
    int32_t* __restrict__ cursor,             // [B] global, init = seg_off[:B]
    int64_t* __restrict__ perm) {             // [>= total]
  extern __shared__ int32_t smem[];           // lcnt[B] + lbase[B]
  int32_t* lcnt = smem;
  int32_t* lbase = smem + B;
  for (int e = threadIdx.x; e < B; e += 256) lcnt[e] = 0;
  __syncthreads();
  const int64_t chunk = (n + gridDim.x - 1) / gridDim.x;
  const int64_t i0 = (int64_t)blockIdx.x * chunk;
  const int64_t i1 = min(n, i0 + chunk);
  for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
    const int64_t sl = lut[node_of_row[i]];
    if (sl >= 0) atomicAdd(&lcnt[sl], 1);
  }
  __syncthreads();
  for (int e = threadIdx.x; e < B; e += 256) {
    const int c = lcnt[e];
    lbase[e] = c ? atomicAdd(&cursor[e], c) : 0;
    lcnt[e] = 0;
  }
  __syncthreads();
  for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
    const int64_t sl = lut[node_of_row[i]];
    if (sl >= 0) {
      const int p = atomicAdd(&lcnt[sl], 1);
      perm[lbase[sl] + p] = i;
    }
  }
}

// ---------------------------------------------------------------------------
// rf_reroute: one-pass row-to-child reassignment after a split batch.
// Replaces the torch lut-gather + nonzero + feature-gather + where chain
// (the byte index_elementwise gathers were ~17% of RFC fit kernel time).
// Training rule: bin <= split_bin goes LEFT (== x < edges[split_bin]).
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(256) void rf_reroute_kernel(
    int64_t* __restrict__ node_of_row,        // [vn] in/out (virtual rows)
    const int64_t* __restrict__ lut2,         // node -> split slot | -1
    const int32_t* __restrict__ sfeat,        // [ns]
    const int32_t* __restrict__ sbin,         // [ns]
    const int64_t* __restrict__ lchild,       // [ns]
    const int64_t* __restrict__ rchild,       // [ns]
    const uint8_t* __restrict__ Xcm,          // [d, n_phys] column-major
    const int32_t* __restrict__ sample,       // [vn] or nullptr
    int64_t n_phys,
    int64_t vn, int64_t d) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < vn; i += stride) {
    const int64_t sl = lut2[node_of_row[i]];
    if (sl < 0) continue;
    const int64_t row = sample ? (int64_t)sample[i]
                               : (i >= n_phys ? i % n_phys : i);
    const uint8_t bin = Xcm[(int64_t)sfeat[sl] * n_phys + row];
    node_of_row[i] = (bin <= (uint8_t)sbin[sl]) ? lchild[sl] : rchild[sl];
  }
}

// ---------------------------------------------------------------------------
// knn_merge_topk: running per-query top-k selection fused with the
// ||q-i||^2 = q_sq + i_sq - 2*dot expansion, consuming a library-GEMM dot
// block ONCE (the torch path materializes d2 and runs multi-pass topk +
// cat/gather merges per item chunk). One wave per query row; each lane owns
// one of 64 candidate slots; tau = current worst kept distance, maintained
// by wave max-reduce. Insertions serialize per wave but decay to rare as tau
// shrinks (expected k*ln(c/k) per row on random-order data).
// Reference: NearestNeighborsMG tiled distance + topk merge (knn.py:763-774).
// ---------------------------------------------------------------------------

__device__ inline float wave_max_f32(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// KEYS = true is the sibling entry point knn_merge_topk_keys: G already holds
// the monotone distance keys of a pairwise_dist block (q_sq / i_sq are unused
// and may be null), everything else — slots, tau, the uniform trip count — is
// the same body.
template <bool KEYS>
__global__ __launch_bounds__(256) void knn_merge_topk_kernel(
    const float* __restrict__ G,     // [nq, c] dot products Q @ I_chunk^T (or keys)
    const float* __restrict__ q_sq,  // [nq]
    const float* __restrict__ i_sq,  // [c]
    int64_t nq, int64_t c, int64_t base,
    float* __restrict__ best_d,      // [nq, 64] slots (+inf live, -inf dead)
    int64_t* __restrict__ best_i) {  // [nq, 64]
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * 4 + wave;
  if (row >= nq) return;

  float cur_d = best_d[row * 64 + lane];
  int64_t cur_i = best_i[row * 64 + lane];
  float tau = wave_max_f32(cur_d);

  const float* g = G + row * c;
  const float qs = KEYS ? 0.0f : q_sq[row];

  // float4 loads are legal only when every row base is 16B-aligned, i.e.
  // c % 4 == 0 (g = G + row*c); otherwise scalar loads
  const bool vec4 = (c & 3) == 0;
  // UNIFORM trip count: every lane of the wave must reach every ballot /
  // shuffle below even when its own j0 has run past c (a per-lane `j0 < c`
  // loop bound left part of the wave outside the evict sequence whenever
  // c % 256 != 0, corrupting tau)
  const int64_t n_iter = (c + 255) / 256;
  for (int64_t it = 0; it < n_iter; ++it) {
    const int64_t j0 = it * 256 + (int64_t)lane * 4;
    float dot4[4], isq4[4];
    if (vec4 && j0 + 3 < c) {
      const float4 gd = *reinterpret_cast<const float4*>(g + j0);
      dot4[0] = gd.x; dot4[1] = gd.y; dot4[2] = gd.z; dot4[3] = gd.w;
      if constexpr (!KEYS) {
        const float4 gi = *reinterpret_cast<const float4*>(i_sq + j0);
        isq4[0] = gi.x; isq4[1] = gi.y; isq4[2] = gi.z; isq4[3] = gi.w;
      }
    } else {
      for (int e = 0; e < 4; ++e) {
        const bool ok = j0 + e < c;
        dot4[e] = ok ? g[j0 + e] : 0.0f;
        if constexpr (!KEYS)
          isq4[e] = ok ? i_sq[j0 + e] : 3.0e38f;  // pushes d2 above any tau
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      // KEYS: a padded column carries key 0 and is masked by j0 + e < c below
      const float d2 = KEYS ? dot4[e] : qs + isq4[e] - 2.0f * dot4[e];
      unsigned long long m = __ballot(d2 < tau && j0 + e < c);
      while (m) {
        const int src = __ffsll((unsigned long long)m) - 1;
        m &= m - 1;
        const float v = __shfl(d2, src, 64);
        if (v >= tau) continue;  // tau shrank since the ballot
        const int col = __shfl((int)(j0 + e), src, 64);
        // evict the current worst slot
        const unsigned long long owners = __ballot(cur_d == tau);
        const int owner = __ffsll((unsigned long long)owners) - 1;
        if (lane == owner) { cur_d = v; cur_i = base + col; }
        tau = wave_max_f32(cur_d);
      }
    }
  }

  best_d[row * 64 + lane] = cur_d;
  best_i[row * 64 + lane] = cur_i;
}

// ---------------------------------------------------------------------------
// pairwise_dist: one [nq, c] block of distance KEYS of queries Q against an
// item chunk, for the metrics that are per-coordinate reductions with no
// GEMM / MFMA form (L1, Linf, Lp, canberra, hamming). It plays the role the
// library GEMM's dot block plays on the euclidean path: knn_merge_topk_keys
// consumes the block once.
//
// 256 threads own one 128x128 output tile; each thread an 8x8 accumulator
// micro-tile split 4+4 in both directions (rows ty*4.. and 64+ty*4.., columns
// tx*4.. and 64+tx*4..) so that each operand fetch of one coordinate is a
// pair of ds_read_b128 whose 16 distinct lane addresses are 16 B apart: 256
// contiguous bytes, one per bank slot (the Q side reads 4 addresses per wave,
// broadcast). d is walked in PD_BK-coordinate chunks staged k-major ([t][row])
// in LDS; the next chunk is fetched to registers while the current one is
// reduced and written to the other LDS buffer, one barrier per chunk.
// Rows past nq / c and coordinates past d are staged as 0 on BOTH sides:
// |0-0| = 0 is the identity of sum and max, 0 == 0 is no hamming mismatch,
// and canberra's 0/0 term is defined as 0.
// The kernel emits the monotone key (sum, max, sum |.|^p, mismatch count);
// the host applies the p-th root / the division by d to the k survivors.
// ---------------------------------------------------------------------------

constexpr int PD_BM = 128;
constexpr int PD_BK = 16;
constexpr int PD_LD = PD_BM + 4;  // row stride: keeps float4 alignment, and the
                                  // transposing stores of one wave 2-way at
                                  // most (free for ds_write_b32)
constexpr int PD_ST = PD_BM * PD_BK / 256;  // staged elements per thread (8)

enum { PD_L1 = 0, PD_LINF = 1, PD_LP = 2, PD_CANBERRA = 3, PD_HAMMING = 4 };

template <int OP>
__device__ inline float pd_accum(float acc, float q, float x, float p) {
  if constexpr (OP == PD_L1) {
    return acc + fabsf(q - x);
  } else if constexpr (OP == PD_LINF) {
    return fmaxf(acc, fabsf(q - x));
  } else if constexpr (OP == PD_LP) {
    // |q-x|^p = 2^(p*log2|q-x|) on the transcendental unit: p is a kernel
    // argument (wave-uniform), no per-lane powf case analysis. log2(0) = -inf
    // and 2^-inf = 0, so equal coordinates (and padding) contribute 0.
    return acc + __builtin_amdgcn_exp2f(p * __builtin_amdgcn_logf(fabsf(q - x)));
  } else if constexpr (OP == PD_CANBERRA) {
    const float den = fabsf(q) + fabsf(x);
    const float t = fabsf(q - x) * __builtin_amdgcn_rcpf(den);
    return acc + (den > 0.0f ? t : 0.0f);  // 0/0 = 0
  } else {
    return acc + (q != x ? 1.0f : 0.0f);
  }
}

template <int OP>
__global__ __launch_bounds__(256) void pairwise_dist_kernel(
    const float* __restrict__ Q,  // [nq, d]
    const float* __restrict__ I,  // [c, d] item chunk
    int64_t nq, int64_t c, int d, float p, int64_t n_it,
    float* __restrict__ out) {    // [nq, c]
  __shared__ __attribute__((aligned(16))) float Qs[2][PD_BK][PD_LD];
  __shared__ __attribute__((aligned(16))) float Is[2][PD_BK][PD_LD];

  const int tid = threadIdx.x;
  const int tx = tid & 15;
  const int ty = tid >> 4;
  const int64_t q0 = ((int64_t)blockIdx.x / n_it) * PD_BM;
  const int64_t i0 = ((int64_t)blockIdx.x % n_it) * PD_BM;

  // staging map: element e of this thread is (row, t) = (lin / BK, lin % BK)
  // with lin = tid + 256 e, i.e. row = (tid >> 4) + 16 e, t = tid & 15:
  // 16 consecutive lanes read 64 contiguous bytes of one row
  const int st = tid & (PD_BK - 1);
  const int sr = tid >> 4;
  float rq[PD_ST], ri[PD_ST];

  auto fetch = [&](int k0) {
    const int t = k0 + st;
    const bool tok = t < d;
#pragma unroll
    for (int e = 0; e < PD_ST; ++e) {
      const int64_t qr = q0 + sr + 16 * e;
      const int64_t ir = i0 + sr + 16 * e;
      rq[e] = (tok && qr < nq) ? Q[qr * d + t] : 0.0f;
      ri[e] = (tok && ir < c) ? I[ir * d + t] : 0.0f;
    }
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int e = 0; e < PD_ST; ++e) {
      Qs[buf][st][sr + 16 * e] = rq[e];
      Is[buf][st][sr + 16 * e] = ri[e];
    }
  };

  float acc[8][8];
#pragma unroll
  for (int a = 0; a < 8; ++a)
#pragma unroll
    for (int b = 0; b < 8; ++b) acc[a][b] = 0.0f;

  const int n_chunks = (d + PD_BK - 1) / PD_BK;
  fetch(0);
  stage(0);
  __syncthreads();
  for (int ch = 0; ch < n_chunks; ++ch) {
    const int buf = ch & 1;
    const bool more = ch + 1 < n_chunks;  // block-uniform
    if (more) fetch((ch + 1) * PD_BK);
    // unrolled by 2 only: a full unroll lets the scheduler hoist every LDS
    // read of the chunk above the arithmetic (256+ live registers, spills)
#pragma unroll 2
    for (int t = 0; t < PD_BK; ++t) {
      const float4 qa = *reinterpret_cast<const float4*>(&Qs[buf][t][ty * 4]);
      const float4 qb = *reinterpret_cast<const float4*>(&Qs[buf][t][64 + ty * 4]);
      const float4 xa = *reinterpret_cast<const float4*>(&Is[buf][t][tx * 4]);
      const float4 xb = *reinterpret_cast<const float4*>(&Is[buf][t][64 + tx * 4]);
      const float qv[8] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w};
      const float xv[8] = {xa.x, xa.y, xa.z, xa.w, xb.x, xb.y, xb.z, xb.w};
#pragma unroll
      for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b) acc[a][b] = pd_accum<OP>(acc[a][b], qv[a], xv[b], p);
    }
    // the other buffer was last read in iteration ch-1, which every thread
    // left through the barrier below
    if (more) stage(buf ^ 1);
    __syncthreads();
  }

  const bool vec4 = (c & 3) == 0;  // every row base of out is then 16B-aligned
#pragma unroll
  for (int a = 0; a < 8; ++a) {
    const int64_t row = q0 + (a < 4 ? ty * 4 + a : 64 + ty * 4 + (a - 4));
    if (row >= nq) continue;
    float* o = out + row * c;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int64_t col = i0 + h * 64 + tx * 4;
      if (vec4 && col + 3 < c) {
        *reinterpret_cast<float4*>(o + col) =
            make_float4(acc[a][4 * h], acc[a][4 * h + 1], acc[a][4 * h + 2], acc[a][4 * h + 3]);
      } else {
#pragma unroll
        for (int b = 0; b < 4; ++b)
          if (col + b < c) o[col + b] = acc[a][4 * h + b];
      }
    }
  }
}

// ---------------------------------------------------------------------------
// csr_pairwise: one [nq, c] block of distance KEYS of CSR query rows against
// an item chunk given in CSC (per column: the chunk-local item rows holding
// it, and their values). It is pairwise_dist's sparse sibling and feeds
// knn_merge_topk_keys the same way.
//
// Every metric served has f(0,0) = 0, so
//   key(q,x) = A_q + B_x + sum_{j in nz(q) & nz(x)} t(q_j, x_j)
// with A_q = sum_j f(q_j,0) and B_x = sum_j f(0,x_j) computed once by the
// caller and t(v,w) = f(v,w) - f(v,0) - f(0,w). Only the intersection is
// walked, Gustavson style: for each nonzero (j, v) of the query row, for each
// (i, w) of column j, acc[i] += t(v, w).
//
// One wave owns one query row (4 rows per block) and keeps the row's acc[c]
// in LDS: zeroed, accumulated, then finished and written to out[row, :] in
// one coalesced pass. The wave takes its row's nonzeros IN ORDER and spreads
// its lanes over the column list: within one nonzero all targets are
// distinct, and nonzeros are sequential, so there are no atomics and the
// f32 sum of every pair has one fixed order (bit-reproducible).
// The row's nonzeros are fetched 64 at a time, one per lane with their column
// bounds, and handed round by shuffles: the colptr lookups of a batch are in
// flight together rather than chained one per nonzero. The batch loops have
// wave-uniform bounds (see knn_merge_topk_kernel); the per-lane loop over a
// column list holds no cross-lane operation.
// Lane use is c*density/64 of a wave when column lists are short: the kernel
// is latency-bound there (profiles/README.md).
// ---------------------------------------------------------------------------

constexpr int CP_CHUNK = 8192;  // 4 rows x 8192 f32 = 128 KB of LDS per block

enum { CP_DOT = 0, CP_L1 = 1, CP_LP = 2, CP_CANBERRA = 3, CP_HAMMING = 4, CP_JACCARD = 5 };

template <int OP>
__device__ inline float cp_term(float v, float w, float p) {
  if constexpr (OP == CP_DOT) {
    return v * w;
  } else if constexpr (OP == CP_L1) {
    return fabsf(v - w) - fabsf(v) - fabsf(w);
  } else if constexpr (OP == CP_LP) {
    // the exp2/log2 form of pd_accum; v == w gives 2^-inf = 0
    return __builtin_amdgcn_exp2f(p * __builtin_amdgcn_logf(fabsf(v - w))) -
           __builtin_amdgcn_exp2f(p * __builtin_amdgcn_logf(fabsf(v))) -
           __builtin_amdgcn_exp2f(p * __builtin_amdgcn_logf(fabsf(w)));
  } else if constexpr (OP == CP_CANBERRA) {
    // stored values are nonzero, so the denominator is positive
    return __fdiv_rn(fabsf(v - w), fabsf(v) + fabsf(w)) - 2.0f;
  } else if constexpr (OP == CP_HAMMING) {
    return (v != w ? 1.0f : 0.0f) - 2.0f;
  } else {
    return 1.0f;
  }
}

template <int OP>
__device__ inline float cp_finish(float a, float b, float acc) {
  if constexpr (OP == CP_DOT) {
    return a + b - 2.0f * acc;
  } else if constexpr (OP == CP_JACCARD) {
    // 1 - acc / (u - acc) with u = nnz(q) + nnz(x), the union being u - acc,
    // as one quotient of exact integers: a single rounding
    const float u = a + b;
    return u > 0.0f ? __fdiv_rn(u - 2.0f * acc, u - acc) : 0.0f;
  } else {
    return a + b + acc;
  }
}

// LDS accesses of one wave execute in order; this only keeps the compiler
// from moving one nonzero's read-modify-writes across the next one's
__device__ inline void cp_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int OP>
__global__ __launch_bounds__(256) void csr_pairwise_kernel(
    const int64_t* __restrict__ q_indptr,  // [nq + 1]
    const int32_t* __restrict__ q_col,     // [nnz_q] column ids
    const float* __restrict__ q_val,       // [nnz_q]
    const int64_t* __restrict__ colptr,    // [d + 1] CSC of the item chunk
    const int32_t* __restrict__ c_row,     // [nnz_c] chunk-local item rows
    const float* __restrict__ c_val,       // [nnz_c]
    const float* __restrict__ A,           // [nq]
    const float* __restrict__ B,           // [c]
    int64_t nq, int c, int d, float p,
    float* __restrict__ out) {             // [nq, c]
  extern __shared__ float cp_acc[];  // [4][c]
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * 4 + wave;
  // before any indptr read; the waves of a block share no barrier below
  if (row >= nq) return;

  float* acc = cp_acc + (size_t)wave * c;
  for (int i = lane; i < c; i += 64) acc[i] = 0.0f;
  cp_wave_sync();

  const int64_t qs = q_indptr[row];
  const int64_t qe = q_indptr[row + 1];
  for (int64_t t0 = qs; t0 < qe; t0 += 64) {
    const int nb = (int)min((int64_t)64, qe - t0);  // wave-uniform
    float v_l = 0.0f;
    int cs_l = 0, ce_l = 0;
    if (lane < nb) {
      const int j = q_col[t0 + lane];
      v_l = q_val[t0 + lane];
      if ((unsigned)j < (unsigned)d) {  // nnz_c < 2^31 is checked on the host
        cs_l = (int)colptr[j];
        ce_l = (int)colptr[j + 1];
      }
    }
    for (int u = 0; u < nb; ++u) {
      const float v = __shfl(v_l, u, 64);
      const int cs = __shfl(cs_l, u, 64);
      const int ce = __shfl(ce_l, u, 64);
      for (int e = cs + lane; e < ce; e += 64) {
        const int i = c_row[e];
        if ((unsigned)i < (unsigned)c) acc[i] += cp_term<OP>(v, c_val[e], p);
      }
      cp_wave_sync();
    }
  }

  const float a = A[row];
  float* o = out + row * c;
  for (int i = lane; i < c; i += 64) o[i] = cp_finish<OP>(a, B[i], acc[i]);
}

// ---------------------------------------------------------------------------
// gather_dists: d2[i][j] = ||A[i] - B[cand[i][j]]||^2 — the nn-descent /
// beam-search hot op (per-row private candidate lists make this a gathered
// row-vs-rows reduction, not a GEMM). One wave per output row: A[i] is
// staged in registers (d/64 floats per lane), each candidate's B row is read
// coalesced by the wave and reduced with a 6-step butterfly. The torch path
// materializes [r, m, d] twice; this reads each gathered row once.
// Reference: cuVS nn_descent / cagra build (umap.py:359-378).
// ---------------------------------------------------------------------------

constexpr int GD_DMAX = 2048;  // register-staged A row: d/64 <= 32 VGPRs

__global__ __launch_bounds__(256) void gather_dists_kernel(
    const float* __restrict__ A,     // [r, d]
    const float* __restrict__ B,     // [n, d]
    const int64_t* __restrict__ cand,  // [r, m]
    int64_t r, int64_t m, int d,
    float* __restrict__ out) {       // [r, m]
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * 4 + wave;
  if (row >= r) return;

  const int nseg = (d + 63) >> 6;  // elements per lane
  float a_reg[GD_DMAX / 64];
  const float* arow = A + row * d;
#pragma unroll 4
  for (int s = 0; s < nseg; ++s) {
    const int idx = s * 64 + lane;
    a_reg[s] = (idx < d) ? arow[idx] : 0.0f;
  }

  const int64_t* crow = cand + row * m;
  for (int64_t j = 0; j < m; ++j) {
    const float* brow = B + crow[j] * d;
    float acc = 0.0f;
#pragma unroll 4
    for (int s = 0; s < nseg; ++s) {
      const int idx = s * 64 + lane;
      const float bv = (idx < d) ? brow[idx] : 0.0f;
      const float diff = a_reg[s] - bv;
      acc = fmaf(diff, diff, acc);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (lane == 0) out[row * m + j] = acc;
  }
}

// ---------------------------------------------------------------------------
// ivf_scan_topk: fused IVF-Flat probed-list scan. One wave per (query, probed
// list) pair: the query row is staged in registers as gather_dists stages A,
// the list's rows (contiguous in the list-sorted item copy) are read
// coalesced and reduced by the 6-step butterfly, and the wave keeps the k
// best in the 64-slot running top-k of knn_merge_topk (lane = slot, tau =
// worst kept key). The key is wave-uniform after the butterfly, so the insert
// test is a uniform branch; only the owner-of-tau ballot remains. No distance
// block is ever materialized. Key, smaller is better:
//   MODE 0: sum (q-x)^2 in the difference form    MODE 1: -q.x
// NSEG (elements per lane, d <= 64*NSEG) is a template parameter so the
// query registers are statically indexed; ROWS list rows are in flight per
// wave before their butterflies to overlap the load latency.
// Reference: cuVS ivf_flat search (knn.py:1485-1491).
// ---------------------------------------------------------------------------

template <int NSEG, int MODE>
__global__ __launch_bounds__(256) void ivf_scan_topk_kernel(
    const float* __restrict__ Q,          // [nq, d]
    const float* __restrict__ Xs,         // [n, d] rows sorted by list
    const int64_t* __restrict__ list_off,   // [nlist + 1]
    const int64_t* __restrict__ pair_q,     // [P]
    const int64_t* __restrict__ pair_list,  // [P]
    const int64_t* __restrict__ pair_out,   // [P] output row of each pair
    int64_t P, int64_t nq, int64_t n, int64_t nlist, int64_t n_out, int d, int k,
    float* __restrict__ part_key,         // [n_out, 64]
    int64_t* __restrict__ part_pos) {     // [n_out, 64] positions into Xs
  constexpr int ROWS = NSEG <= 4 ? 4 : (NSEG <= 16 ? 2 : 1);
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int64_t p = (int64_t)blockIdx.x * 4 + wave;
  if (p >= P) return;
  const int64_t qi = pair_q[p];
  const int64_t li = pair_list[p];
  const int64_t oi = pair_out[p];
  // a malformed work item is dropped, never dereferenced (wave-uniform)
  if (qi < 0 || qi >= nq || li < 0 || li >= nlist || oi < 0 || oi >= n_out) return;
  int64_t lo = list_off[li], hi = list_off[li + 1];
  lo = lo < 0 ? 0 : lo;
  hi = hi > n ? n : hi;

  float q_reg[NSEG];
  const float* qrow = Q + qi * d;
#pragma unroll
  for (int s = 0; s < NSEG; ++s) {
    const int idx = s * 64 + lane;
    q_reg[s] = (idx < d) ? qrow[idx] : 0.0f;
  }

  // lanes >= k are dead slots (-inf never owns tau); live slots start empty
  float cur_k = lane < k ? INFINITY : -INFINITY;
  int64_t cur_p = -1;
  float tau = INFINITY;

  for (int64_t j0 = lo; j0 < hi; j0 += ROWS) {
    float acc[ROWS];
#pragma unroll
    for (int u = 0; u < ROWS; ++u) {
      acc[u] = 0.0f;
      if (j0 + u < hi) {  // wave-uniform
        const float* xrow = Xs + (j0 + u) * d;
#pragma unroll
        for (int s = 0; s < NSEG; ++s) {
          const int idx = s * 64 + lane;
          const float xv = (idx < d) ? xrow[idx] : 0.0f;
          if (MODE == 0) {
            const float diff = q_reg[s] - xv;
            acc[u] = fmaf(diff, diff, acc[u]);
          } else {
            acc[u] = fmaf(q_reg[s], xv, acc[u]);
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < ROWS; ++u) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) acc[u] += __shfl_xor(acc[u], off, 64);
    }
#pragma unroll
    for (int u = 0; u < ROWS; ++u) {
      // every lane holds the same sum after the butterfly; reading it from
      // the first lane lets the compiler see the insert test as uniform
      const float key = __int_as_float(__builtin_amdgcn_readfirstlane(
          __float_as_int(MODE == 0 ? acc[u] : -acc[u])));
      if (j0 + u < hi && key < tau) {  // no candidate ballot needed
        const unsigned long long owners = __ballot(cur_k == tau);
        const int owner = __ffsll((unsigned long long)owners) - 1;
        if (lane == owner) { cur_k = key; cur_p = j0 + u; }
        tau = __int_as_float(__builtin_amdgcn_readfirstlane(
            __float_as_int(wave_max_f32(cur_k))));
      }
    }
  }

  part_key[oi * 64 + lane] = cur_k;
  part_pos[oi * 64 + lane] = cur_p;
}

// ---------------------------------------------------------------------------
// ivfpq_scan_topk: fused IVF-PQ ADC scan. One 256-thread block per (query,
// probed list) pair, because the pair's lookup table lives in LDS and is
// shared by the block's four waves:
//   1. stage q - C[l] (MODE 0) or q (MODE 1) in LDS and build
//        MODE 0: LUT[m][c] = sum_j (qres[m*ds+j] - cb[m][c][j])^2
//        MODE 1: LUT[m][c] = -sum_j q[m*ds+j] * cb[m][c][j]   (+ base -q.C[l])
//      in the difference form of ivf_scan_topk. Thread t owns code
//      t % ncodes and walks m from t / ncodes in steps of 256 / ncodes, so
//      one step of the block reads a contiguous run of the codebooks.
//   2. each lane takes one list row per trip (a wave 64 consecutive rows,
//      the block 256), reads its M code bytes — as dwords when the row stride
//      and base allow (`vec4`; the stride may be padded past M), else as
//      bytes — and sums LUT[m][code & (ncodes-1)]: the mask keeps every index
//      inside its LUT row whatever the bytes hold.
//   3. keys are per lane, so insertion is the candidate-ballot loop of
//      knn_merge_topk with the same wave-uniform trip count. A lane owns
//      SLOTS statically indexed slots (slot s*64+lane, live below k_cand,
//      dead = -inf otherwise); each wave keeps the best k_cand of its quarter
//      of the rows, waves 1-3 park theirs in LDS (key + i32 offset from the
//      list start) and wave 0 merges them through the same insert.
// The LUT gathers of step 2 hit random banks and will conflict; that cost is
// accepted here and has not been measured.
// Dynamic LDS: LUT M*ncodes*4 | query d*4 (padded to 16 B) | 3*64*SLOTS*8.
// Reference: cuVS ivf_pq search (knn.py:1512-1515).
// ---------------------------------------------------------------------------

constexpr int64_t PQ_LDS_BUDGET = 144 * 1024;

static inline int64_t ivfpq_lds_bytes(int64_t M, int64_t ncodes, int64_t d, int64_t slots) {
  return M * ncodes * 4 + ((d + 3) / 4) * 16 + 3 * 64 * slots * 8;
}

// one candidate-ballot insert round: every lane of the wave must call it
template <int SLOTS>
__device__ inline void pq_insert(float key, int pos, bool valid, float (&cur_k)[SLOTS],
                                 int (&cur_p)[SLOTS], float& tau) {
  unsigned long long m = __ballot(valid && key < tau);
  while (m) {
    const int src = __ffsll((unsigned long long)m) - 1;
    m &= m - 1;
    const float v = __shfl(key, src, 64);
    if (v >= tau) continue;  // tau shrank since the ballot
    const int vp = __shfl(pos, src, 64);
    float lmax = cur_k[0];
#pragma unroll
    for (int s = 1; s < SLOTS; ++s) lmax = fmaxf(lmax, cur_k[s]);
    // evict the current worst slot
    const unsigned long long owners = __ballot(lmax == tau);
    const int owner = __ffsll((unsigned long long)owners) - 1;
    if ((int)(threadIdx.x & 63) == owner) {
      bool done = false;
#pragma unroll
      for (int s = 0; s < SLOTS; ++s) {
        if (!done && cur_k[s] == tau) { cur_k[s] = v; cur_p[s] = vp; done = true; }
      }
    }
    lmax = cur_k[0];
#pragma unroll
    for (int s = 1; s < SLOTS; ++s) lmax = fmaxf(lmax, cur_k[s]);
    tau = wave_max_f32(lmax);
  }
}

template <int SLOTS, int MODE>
__global__ __launch_bounds__(256) void ivfpq_scan_topk_kernel(
    const float* __restrict__ Q,            // [nq, d]
    const float* __restrict__ C,            // [nlist, d]
    const float* __restrict__ cb,           // [M, ncodes, ds]
    const uint8_t* __restrict__ codes,      // [n, stride] rows sorted by list
    const int64_t* __restrict__ list_off,   // [nlist + 1]
    const int64_t* __restrict__ pair_q,     // [P]
    const int64_t* __restrict__ pair_list,  // [P]
    const int64_t* __restrict__ pair_out,   // [P] output row of each pair
    int64_t P, int64_t nq, int64_t n, int64_t nlist, int64_t n_out, int d, int M,
    int ncodes, int ds, int64_t stride, int vec4, int k_cand,
    float* __restrict__ part_key,           // [n_out, 64*SLOTS]
    int64_t* __restrict__ part_pos) {       // [n_out, 64*SLOTS] positions into codes
  extern __shared__ __attribute__((aligned(16))) unsigned char pq_smem[];
  float* lut = reinterpret_cast<float*>(pq_smem);
  float* qs = lut + (size_t)M * ncodes;
  float* mk = qs + (size_t)((d + 3) / 4) * 4;
  int* mp = reinterpret_cast<int*>(mk + 3 * 64 * SLOTS);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int64_t p = blockIdx.x;
  if (p >= P) return;
  const int64_t qi = pair_q[p];
  const int64_t li = pair_list[p];
  const int64_t oi = pair_out[p];
  // a malformed work item is dropped, never dereferenced (block-uniform, so
  // the barriers below are reached by all threads or none)
  if (qi < 0 || qi >= nq || li < 0 || li >= nlist || oi < 0 || oi >= n_out) return;
  int64_t lo = list_off[li], hi = list_off[li + 1];
  lo = lo < 0 ? 0 : (lo > n ? n : lo);
  hi = hi < 0 ? 0 : (hi > n ? n : hi);
  // offsets from the list start are kept as i32
  if (hi - lo > 0x7fffffffLL) hi = lo + 0x7fffffffLL;

  float cur_k[SLOTS];
  int cur_p[SLOTS];
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) {
    // slots >= k_cand are dead (-inf never owns tau); live slots start empty
    cur_k[s] = (s * 64 + lane < k_cand) ? INFINITY : -INFINITY;
    cur_p[s] = -1;
  }

  if (hi > lo) {  // block-uniform
    const float* qrow = Q + qi * d;
    const float* crow = C + li * d;
    for (int i = tid; i < d; i += 256)
      qs[i] = MODE == 0 ? qrow[i] - crow[i] : qrow[i];
    __syncthreads();

    // ---- phase 1: the pair's LUT
    {
      const int code = tid & (ncodes - 1);
      const int mstep = 256 / ncodes;
      for (int m = tid / ncodes; m < M; m += mstep) {
        const float* cv = cb + ((size_t)m * ncodes + code) * ds;
        const float* qv = qs + m * ds;
        float acc = 0.0f;
        if ((ds & 3) == 0) {  // cb base is 16 B aligned (checked on the host)
          for (int j = 0; j < ds; j += 4) {
            const float4 c4 = *reinterpret_cast<const float4*>(cv + j);
            const float cj[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              if (MODE == 0) {
                const float diff = qv[j + e] - cj[e];
                acc = fmaf(diff, diff, acc);
              } else {
                acc = fmaf(qv[j + e], cj[e], acc);
              }
            }
          }
        } else {
          for (int j = 0; j < ds; ++j) {
            if (MODE == 0) {
              const float diff = qv[j] - cv[j];
              acc = fmaf(diff, diff, acc);
            } else {
              acc = fmaf(qv[j], cv[j], acc);
            }
          }
        }
        lut[m * ncodes + code] = MODE == 0 ? acc : -acc;
      }
    }
    // MODE 1: the pair's base -q.C[l], computed by every wave for itself
    float base = 0.0f;
    if (MODE == 1) {
      for (int i = lane; i < d; i += 64) base = fmaf(qs[i], crow[i], base);
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) base += __shfl_xor(base, off, 64);
      base = -base;
    }
    __syncthreads();

    // ---- phase 2 + 3: scan the list, keep the wave's best k_cand
    float tau = INFINITY;
    const int cmask = ncodes - 1;
    const int nword = M >> 2, ntail = M & 3;
    const int64_t len = hi - lo;
    // UNIFORM trip count (see knn_merge_topk_kernel): lanes past the end of
    // the list still take part in every ballot and shuffle
    const int64_t n_iter = (len + 255) / 256;
    for (int64_t it = 0; it < n_iter; ++it) {
      const int64_t off = it * 256 + wave * 64 + lane;
      const bool valid = off < len;
      float key = INFINITY;
      if (valid) {
        const uint8_t* row = codes + (lo + off) * stride;
        float a0 = base, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
        if (vec4) {
          const uint32_t* row4 = reinterpret_cast<const uint32_t*>(row);
          const float* lrow = lut;
#pragma unroll 4
          for (int w = 0; w < nword; ++w) {
            const uint32_t v = row4[w];
            a0 += lrow[(int)(v & 0xff) & cmask];
            a1 += lrow[ncodes + ((int)((v >> 8) & 0xff) & cmask)];
            a2 += lrow[2 * ncodes + ((int)((v >> 16) & 0xff) & cmask)];
            a3 += lrow[3 * ncodes + ((int)(v >> 24) & cmask)];
            lrow += 4 * ncodes;
          }
          if (ntail) {  // stride % 4 == 0 and stride >= M: the word is in the row
            const uint32_t v = row4[nword];
            a0 += lrow[(int)(v & 0xff) & cmask];
            if (ntail > 1) a1 += lrow[ncodes + ((int)((v >> 8) & 0xff) & cmask)];
            if (ntail > 2) a2 += lrow[2 * ncodes + ((int)((v >> 16) & 0xff) & cmask)];
          }
        } else {
          int m = 0;
          for (; m + 3 < M; m += 4) {
            a0 += lut[m * ncodes + ((int)row[m] & cmask)];
            a1 += lut[(m + 1) * ncodes + ((int)row[m + 1] & cmask)];
            a2 += lut[(m + 2) * ncodes + ((int)row[m + 2] & cmask)];
            a3 += lut[(m + 3) * ncodes + ((int)row[m + 3] & cmask)];
          }
          for (; m < M; ++m) a0 += lut[m * ncodes + ((int)row[m] & cmask)];
        }
        key = (a0 + a1) + (a2 + a3);
      }
      pq_insert<SLOTS>(key, (int)off, valid, cur_k, cur_p, tau);
    }

    // ---- merge: waves 1-3 park their slots, wave 0 inserts them
    if (wave > 0) {
#pragma unroll
      for (int s = 0; s < SLOTS; ++s) {
        mk[(wave - 1) * 64 * SLOTS + s * 64 + lane] = cur_k[s];
        mp[(wave - 1) * 64 * SLOTS + s * 64 + lane] = cur_p[s];
      }
    }
    __syncthreads();
    if (wave == 0) {
      for (int i = 0; i < 3 * SLOTS; ++i) {
        const float key = mk[i * 64 + lane];
        const int pos = mp[i * 64 + lane];
        // dead and empty slots carry position -1
        pq_insert<SLOTS>(key, pos, pos >= 0, cur_k, cur_p, tau);
      }
    }
  }

  if (wave == 0) {
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
      part_key[oi * (64 * SLOTS) + s * 64 + lane] = cur_k[s];
      part_pos[oi * (64 * SLOTS) + s * 64 + lane] =
          cur_p[s] >= 0 ? lo + (int64_t)cur_p[s] : (int64_t)-1;
    }
  }
}

// ---------------------------------------------------------------------------
// cagra_search: fused graph beam search, one 256-thread block per query. The
// whole search state lives in LDS, so a search is one launch instead of a
// chain of topk / gather / cat / sort launches per hop:
//   buf     u64 [pow2 >= max(ns, itopk + search_width*deg)]: the sorted list
//           in buf[0, L) and this iteration's candidates behind it. An entry
//           is (f32 key bits << 32) | id; non-negative f32 keys order as
//           unsigned integers, so the u64 order is the (key, id) order. Bit 31
//           of the low word is the entry's "expanded" flag; ids are < 2^31
//           and every compare masks the flag out, so it rides along without
//           entering the order.
//   hash    i32 [2^hash_bits]: the visited filter, open addressing with
//           linear probing, -1 = empty.
//   parents i32 [min(search_width, itopk)], then the query row (f32).
// Seeding and every iteration share one pipeline: gather ids (seeds, or the
// parents' graph rows), drop ids outside [0, n) and ids the filter has seen
// (one atomicCAS per id, so a duplicate inside one iteration is dropped too),
// key the survivors once with a 16-lane team per candidate row (float4 loads
// when d % 4 == 0, 4-step butterfly), then one bitonic sort of list +
// candidates and a trim to itopk. The candidates reach buf in atomic order,
// which varies from run to run; the sort erases that, and the candidate SET
// and every count depend only on the inputs.
// Before an iteration that could take the filter past half full it is cleared
// and refilled with the list's ids. A node keyed before a reset can be keyed
// again but sorts behind the list's worst entry, which never gets worse, so
// resets change stats[1] and stats[2] only.
// stats = (iterations that expanded a parent, keys computed, filter resets).
// LDS trade, not measured against alternatives: with hash_bits = 0 the
// wrapper doubles the filter from its minimum 2*max(itopk+search_width*deg,
// ns) while the block stays under CG_LDS_TARGET = 32 KiB, i.e. at least five
// blocks (20 waves) per CU of 160 KiB. The search is a chain of dependent
// gathers, so resident waves hide its latency; a bigger filter would only
// save the re-keying after a reset. At the ANN bench shape (d 300, itopk
// 128, width 16, deg 48) that is 8 KiB buf + 16 KiB filter + 1.3 KiB.
// Reference: cuVS cagra single-CTA search (knn.py:1521-1524).
// ---------------------------------------------------------------------------

constexpr int64_t CG_LDS_BUDGET = 144 * 1024;  // hard limit, as ivfpq_scan_topk
constexpr int64_t CG_LDS_TARGET = 32 * 1024;   // hash_bits = 0 stays under this
constexpr unsigned long long CG_ORDER_MASK = ~(1ull << 31);
constexpr unsigned long long CG_EXPANDED = 1ull << 31;

static inline int64_t cg_pow2_ceil(int64_t v) {
  int64_t p = 1;
  while (p < v) p <<= 1;
  return p;
}

static inline int64_t cagra_lds_bytes(int64_t d, int64_t itopk, int64_t width, int64_t deg,
                                      int64_t ns, int64_t slots) {
  const int64_t buf = cg_pow2_ceil(std::max<int64_t>(ns, itopk + width * deg));
  const int64_t pcap = (std::min<int64_t>(width, itopk) + 3) / 4 * 4;
  return buf * 8 + slots * 4 + pcap * 4 + (d + 3) / 4 * 16;
}

// true when `id` was not in the filter yet (and now is). The probe count is
// bounded by the table size; the load stays <= 1/2, so the bound is never hit.
__device__ inline bool cg_visit(int* hash, unsigned mask, int shift, int id) {
  unsigned h = ((unsigned)id * 2654435761u) >> shift;
  for (unsigned probe = 0; probe <= mask; ++probe) {
    const int old = atomicCAS(&hash[h & mask], -1, id);
    if (old == -1) return true;
    if (old == id) return false;
    ++h;
  }
  return false;
}

// keys of buf[L, L + ncand) (ids on entry), the pad up to the next power of
// two, and the sort of buf[0, P2). Returns the new list length. Every thread
// of the block must call it with the same L and ncand.
__device__ inline int cg_key_sort_trim(unsigned long long* buf, const float* qs,
                                       const float* __restrict__ X, int d, bool vec,
                                       int L, int ncand, int itopk) {
  const int tid = threadIdx.x;
  const int team = tid >> 4, tl = tid & 15;
  for (int c0 = 0; c0 < ncand; c0 += 16) {  // block-uniform trip count
    const int c = c0 + team;
    const bool valid = c < ncand;
    const int id = valid ? (int)(buf[L + c] & 0x7fffffffull) : 0;
    float acc = 0.0f;
    if (valid) {
      if (vec) {
        const int nvec = d >> 2;
        const float4* x4 = reinterpret_cast<const float4*>(X + (size_t)id * d);
        const float4* q4 = reinterpret_cast<const float4*>(qs);
#pragma unroll 4
        for (int v = tl; v < nvec; v += 16) {
          const float4 x = x4[v];
          const float4 q = q4[v];
          const float d0 = q.x - x.x, d1 = q.y - x.y, d2 = q.z - x.z, d3 = q.w - x.w;
          acc = fmaf(d0, d0, acc);
          acc = fmaf(d1, d1, acc);
          acc = fmaf(d2, d2, acc);
          acc = fmaf(d3, d3, acc);
        }
      } else {
        const float* xr = X + (size_t)id * d;
#pragma unroll 4
        for (int i = tl; i < d; i += 16) {
          const float diff = qs[i] - xr[i];
          acc = fmaf(diff, diff, acc);
        }
      }
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (valid && tl == 0)
      buf[L + c] = ((unsigned long long)__float_as_uint(acc) << 32) | (unsigned)id;
  }
  const int total = L + ncand;
  int P2 = 1;
  while (P2 < total) P2 <<= 1;
  for (int i = total + tid; i < P2; i += 256) buf[i] = ~0ull;
  __syncthreads();
  if (ncand > 0) {  // block-uniform; the list alone is already sorted
    for (int k2 = 2; k2 <= P2; k2 <<= 1) {
      for (int j = k2 >> 1; j > 0; j >>= 1) {
        for (int i = tid; i < (P2 >> 1); i += 256) {
          const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1));
          const int hi = lo | j;
          const bool asc = (lo & k2) == 0;
          const unsigned long long a = buf[lo], b = buf[hi];
          if (((a & CG_ORDER_MASK) > (b & CG_ORDER_MASK)) == asc) {
            buf[lo] = b;
            buf[hi] = a;
          }
        }
        __syncthreads();
      }
    }
  }
  return total < itopk ? total : itopk;
}

__global__ __launch_bounds__(256) void cagra_search_kernel(
    const float* __restrict__ Q,    // [nq, d]
    const float* __restrict__ X,    // [n, d]
    const int* __restrict__ G,      // [n, deg]
    const int* __restrict__ seeds,  // [nq, ns]
    int n, int d, int deg, int ns, int k, int itopk, int width, int max_it,
    int hash_bits, int vec,
    float* __restrict__ out_key,    // [nq, k]
    int* __restrict__ out_id,       // [nq, k]
    int* __restrict__ stats) {      // [nq, 3]
  extern __shared__ __attribute__((aligned(16))) unsigned char cg_smem[];
  __shared__ int s_np, s_ncand;
  int bufcap = 1;
  {
    const int need = ns > itopk + width * deg ? ns : itopk + width * deg;
    while (bufcap < need) bufcap <<= 1;
  }
  const int slots = 1 << hash_bits;
  const int pcap = ((width < itopk ? width : itopk) + 3) & ~3;
  unsigned long long* buf = reinterpret_cast<unsigned long long*>(cg_smem);
  int* hash = reinterpret_cast<int*>(buf + bufcap);
  int* parents = hash + slots;
  float* qs = reinterpret_cast<float*>(parents + pcap);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int64_t qi = blockIdx.x;
  const unsigned hmask = (unsigned)slots - 1u;
  const int hshift = 32 - hash_bits;
  const int half = slots >> 1;

  // ---- seeding
  for (int i = tid; i < d; i += 256) qs[i] = Q[qi * d + i];
  for (int i = tid; i < slots; i += 256) hash[i] = -1;
  if (tid == 0) s_ncand = 0;
  __syncthreads();
  for (int t = tid; t < ns; t += 256) {
    const int id = seeds[qi * ns + t];
    if (id >= 0 && id < n && cg_visit(hash, hmask, hshift, id))
      buf[atomicAdd(&s_ncand, 1)] = (unsigned)id;
  }
  __syncthreads();
  int ncand = s_ncand;
  int L = cg_key_sort_trim(buf, qs, X, d, vec != 0, 0, ncand, itopk);
  int hcount = ncand, evals = ncand, iters = 0, resets = 0;

  for (int it = 0; it < max_it; ++it) {
    // ---- filter reset (every quantity here is block-uniform)
    const int after = hcount + width * deg < n ? hcount + width * deg : n;
    if (after > half) {
      for (int i = tid; i < slots; i += 256) hash[i] = -1;
      __syncthreads();
      for (int i = tid; i < L; i += 256)
        cg_visit(hash, hmask, hshift, (int)(buf[i] & 0x7fffffffull));
      hcount = L;
      ++resets;
      // the parent pick below rewrites buf entries these inserts read
      __syncthreads();
    }
    // ---- 1. parents: the first `width` unexpanded entries in list order
    if (wave == 0) {
      int taken = 0;
      for (int base = 0; base < L && taken < width; base += 64) {
        const int i = base + lane;
        const bool un = i < L && !(buf[i] & CG_EXPANDED);
        const unsigned long long m = __ballot(un);
        const int r = taken + __popcll(m & ((1ull << lane) - 1ull));
        if (un && r < width) {
          parents[r] = (int)(buf[i] & 0x7fffffffull);
          buf[i] |= CG_EXPANDED;
        }
        taken += __popcll(m);
      }
      if (lane == 0) {
        s_np = taken < width ? taken : width;
        s_ncand = 0;
      }
    }
    __syncthreads();
    const int np = s_np;
    if (np == 0) break;  // nothing left to expand
    ++iters;
    // ---- 2. candidates: the parents' valid, unvisited graph entries
    for (int t = tid; t < np * deg; t += 256) {
      const int p = parents[t / deg];
      const int id = G[(size_t)p * deg + (t % deg)];
      if (id >= 0 && id < n && cg_visit(hash, hmask, hshift, id))
        buf[L + atomicAdd(&s_ncand, 1)] = (unsigned)id;
    }
    __syncthreads();
    ncand = s_ncand;
    hcount += ncand;
    evals += ncand;
    // ---- 3. key, merge, trim
    L = cg_key_sort_trim(buf, qs, X, d, vec != 0, L, ncand, itopk);
  }

  for (int i = tid; i < k; i += 256) {
    const unsigned long long e = buf[i < L ? i : 0];
    out_key[qi * k + i] = i < L ? __uint_as_float((unsigned)(e >> 32)) : INFINITY;
    out_id[qi * k + i] = i < L ? (int)(e & 0x7fffffffull) : -1;
  }
  if (tid == 0) {
    stats[qi * 3 + 0] = iters;
    stats[qi * 3 + 1] = evals;
    stats[qi * 3 + 2] = resets;
  }
}

// ---------------------------------------------------------------------------
// cagra_prune: rank-based detour counting and reordering of a kNN graph
// (cuVS cagra's graph optimisation, first half). G is [n, D] item ids, row u
// in ascending distance order. Integer-only, so the result does not depend on
// the order in which the LDS atomics land:
//   entry j of row u is dead if G[u][j] == u or repeats an earlier entry;
//   detour[u][j] = #{ i < j : i live, G[u][j] in set(G[G[u][i]]) }, -1 if dead;
//   P[u] = live entries by (detour, j), first D_out, padded with u.
// One wave per node in a 64-thread block: every phase boundary is then a
// barrier of that wave alone, and no wave waits for another node's live
// count. Per node, in LDS (ints): the row, an open-addressed id -> first rank
// table of 2 * pow2ceil(D) slots (linear probing, -1 = empty, load <= 1/2),
// cnt[D] and last[D], the live ranks compacted in order, and pow2ceil(D) sort
// keys (detour << 9 | j). For each live i in rank order the lanes read
// neighbour i's row coalesced and probe the table; a hit at rank j > i swaps
// i into last[j] and bumps cnt[j] unless i was already there, so a neighbour
// that holds the id twice counts once. That needs the table updates of one i
// to precede those of the next: the loads of CP_BATCH neighbour rows are
// issued together (they are dependent gathers), the probes then run one row
// after the other in program order, and a wave's LDS operations complete in
// order. An id outside [0, n) is never dereferenced (it is treated as dead);
// ids in range are the caller's precondition.
// Reference: cuVS cagra::optimize (knn.py:978-982).
// ---------------------------------------------------------------------------

constexpr int CP_MAX_D = 256;
constexpr int CP_BATCH = 4;
constexpr int CP_DEAD_KEY = 0x7fffffff;

static inline int64_t cagra_prune_lds_bytes(int64_t D) {
  const int64_t p2 = cg_pow2_ceil(D);
  return (4 * D + 5 * p2) * 4;  // row, cnt, last, liv | 2 tables of 2*p2 | keys
}

// slot of `id` in the table, or -1. Read-only; an empty slot ends the probe.
__device__ inline int cp_find(const int* tab_id, unsigned mask, int shift, int id) {
  unsigned h = ((unsigned)id * 2654435761u) >> shift;
  for (unsigned probe = 0; probe <= mask; ++probe) {
    const int s = (int)(h & mask);
    const int got = tab_id[s];
    if (got == id) return s;
    if (got == -1) return -1;
    ++h;
  }
  return -1;
}

template <int CH>  // CH = ceil(D / 64) row entries per lane
__global__ __launch_bounds__(64) void cagra_prune_kernel(
    const int* __restrict__ G,   // [n, D]
    int n, int D, int D_out, int p2, int tab_bits,
    int* __restrict__ P,         // [n, D_out]
    int* __restrict__ detour) {  // [n, D]
  extern __shared__ __attribute__((aligned(16))) unsigned char cp_smem[];
  int* row = reinterpret_cast<int*>(cp_smem);
  int* cnt = row + D;
  int* last = cnt + D;
  int* liv = last + D;
  int* tab_id = liv + D;
  const int slots = 2 * p2;
  int* tab_rank = tab_id + slots;
  int* keys = tab_rank + slots;

  const int lane = threadIdx.x;
  const unsigned mask = (unsigned)slots - 1u;
  const int shift = 32 - tab_bits;

  for (int64_t u64 = blockIdx.x; u64 < n; u64 += gridDim.x) {
    const int u = (int)u64;
    // ---- 0. the row, cleared counters and table
    for (int j = lane; j < D; j += 64) {
      row[j] = G[(size_t)u * D + j];
      cnt[j] = 0;
      last[j] = -1;
    }
    for (int s = lane; s < slots; s += 64) {
      tab_id[s] = -1;
      tab_rank[s] = CP_DEAD_KEY;
    }
    __syncthreads();
    // ---- 1. id -> first rank
    for (int j = lane; j < D; j += 64) {
      const int id = row[j];
      if (id == u || id < 0 || id >= n) continue;
      unsigned h = ((unsigned)id * 2654435761u) >> shift;
      for (unsigned probe = 0; probe <= mask; ++probe) {
        const int s = (int)(h & mask);
        const int old = atomicCAS(&tab_id[s], -1, id);
        if (old == -1 || old == id) {
          atomicMin(&tab_rank[s], j);
          break;
        }
        ++h;
      }
    }
    __syncthreads();
    // ---- 2. live ranks, compacted in order; a dead entry reports -1
    int nlive = 0;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int j = c * 64 + lane;
      bool live = false;
      if (j < D) {
        const int id = row[j];
        if (id != u && id >= 0 && id < n) {
          const int s = cp_find(tab_id, mask, shift, id);
          live = s >= 0 && tab_rank[s] == j;
        }
        if (!live) cnt[j] = -1;
      }
      const unsigned long long m = __ballot(live);
      if (live) liv[nlive + __popcll(m & ((1ull << lane) - 1ull))] = j;
      nlive += __popcll(m);
    }
    __syncthreads();
    // ---- 3. detour counts
    for (int t0 = 0; t0 < nlive; t0 += CP_BATCH) {  // wave-uniform trip count
      int vals[CP_BATCH][CH];
      int rank_i[CP_BATCH];
#pragma unroll
      for (int b = 0; b < CP_BATCH; ++b) {
        const bool on = t0 + b < nlive;
        rank_i[b] = on ? liv[t0 + b] : -1;
        const int nb = on ? row[rank_i[b]] : 0;
        const int* nrow = G + (size_t)nb * D;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
          const int e = c * 64 + lane;
          vals[b][c] = (on && e < D) ? nrow[e] : -1;
        }
      }
#pragma unroll
      for (int b = 0; b < CP_BATCH; ++b) {
        const int i = rank_i[b];
#pragma unroll
        for (int c = 0; c < CH; ++c) {
          const int id = vals[b][c];
          if (id < 0 || id >= n) continue;
          const int s = cp_find(tab_id, mask, shift, id);
          if (s < 0) continue;
          const int j = tab_rank[s];
          if (j > i && atomicExch(&last[j], i) != i) atomicAdd(&cnt[j], 1);
        }
      }
    }
    __syncthreads();
    // ---- 4. detour out, then the live entries by (detour, rank)
    for (int j = lane; j < D; j += 64) detour[(size_t)u * D + j] = cnt[j];
    for (int j = lane; j < p2; j += 64)
      keys[j] = (j < D && cnt[j] >= 0) ? ((cnt[j] << 9) | j) : CP_DEAD_KEY;
    __syncthreads();
    for (int k2 = 2; k2 <= p2; k2 <<= 1) {
      for (int jj = k2 >> 1; jj > 0; jj >>= 1) {
        for (int i = lane; i < (p2 >> 1); i += 64) {
          const int lo = ((i & ~(jj - 1)) << 1) | (i & (jj - 1));
          const int hi = lo | jj;
          const bool asc = (lo & k2) == 0;
          const int a = keys[lo], b = keys[hi];
          if ((a > b) == asc) {
            keys[lo] = b;
            keys[hi] = a;
          }
        }
        __syncthreads();
      }
    }
    for (int k = lane; k < D_out; k += 64) {
      const int key = keys[k];
      P[(size_t)u * D_out + k] = key == CP_DEAD_KEY ? u : row[key & 511];
    }
    __syncthreads();  // the next node rewrites everything
  }
}

// ---------------------------------------------------------------------------
// CSR GLM kernels (the reference's LogisticRegressionMG sparse path,
// classification.py:960-966, runs cuML SpMM; torch/rocSPARSE here spent its
// time in f64 index_add column stats, a 400M-pair radix-sort transpose and
// a generic csrmm — these three passes replace all of it):
//  - csr_fwd:        scores[n,C] = A @ WT   (thread per row, ~nnz/row loop)
//  - csr_grad:       grad[C,d]  += val * resid[row,C] scattered by column
//                    (2048-way atomic fan-out pipelines fine; removes the
//                    pre-transposed CSR entirely)
//  - csr_col_moments: per-column sum / sum-of-squares in one pass
// ---------------------------------------------------------------------------

template <typename IdxT>
__global__ __launch_bounds__(256) void csr_fwd_kernel(
    const IdxT* __restrict__ indptr, const IdxT* __restrict__ indices,
    const float* __restrict__ vals, const float* __restrict__ WT,  // [d, C]
    int64_t n, int C, float* __restrict__ scores) {                // [n, C]
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    float acc[32];
    for (int c = 0; c < C; ++c) acc[c] = 0.0f;
    const int64_t e0 = (int64_t)indptr[i], e1 = (int64_t)indptr[i + 1];
    for (int64_t j = e0; j < e1; ++j) {
      const float v = vals[j];
      const float* wrow = WT + (int64_t)indices[j] * C;
      for (int c = 0; c < C; ++c) acc[c] = fmaf(v, wrow[c], acc[c]);
    }
    for (int c = 0; c < C; ++c) scores[i * C + c] = acc[c];
  }
}

template <typename IdxT>
__global__ __launch_bounds__(256) void csr_grad_kernel(
    const IdxT* __restrict__ indptr, const IdxT* __restrict__ indices,
    const float* __restrict__ vals, const float* __restrict__ resid,  // [n, C]
    int64_t n, int64_t d, int C, int use_lds,
    float* __restrict__ grad) {          // [C, d]
  // grad is tiny ([C, d] ~ KBs): accumulate per BLOCK in LDS and flush once
  // — 400M chip-wide global atomics onto 2048 words ran at ~8 G/s (48 ms
  // per iteration); LDS-privatized they cost ~5 ms
  extern __shared__ float g_s[];
  const int64_t cd = (int64_t)C * d;
  if (use_lds) {
    for (int64_t e = threadIdx.x; e < cd; e += 256) g_s[e] = 0.0f;
    __syncthreads();
  }
  float* acc = use_lds ? g_s : grad;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    float r[32];
    for (int c = 0; c < C; ++c) r[c] = resid[i * C + c];
    const int64_t e0 = (int64_t)indptr[i], e1 = (int64_t)indptr[i + 1];
    for (int64_t j = e0; j < e1; ++j) {
      const float v = vals[j];
      const int64_t col = (int64_t)indices[j];
      for (int c = 0; c < C; ++c) atomicAdd(&acc[(int64_t)c * d + col], v * r[c]);
    }
  }
  if (use_lds) {
    __syncthreads();
    for (int64_t e = threadIdx.x; e < cd; e += 256)
      if (g_s[e] != 0.0f) atomicAdd(&grad[e], g_s[e]);
  }
}

template <typename IdxT>
__global__ __launch_bounds__(256) void csr_col_moments_kernel(
    const IdxT* __restrict__ indices, const float* __restrict__ vals,
    int64_t nnz, int64_t d, double* __restrict__ out) {  // [2, d] sum, sumsq
  extern __shared__ double cm_s[];  // [2, d] per-block
  for (int64_t e = threadIdx.x; e < 2 * d; e += 256) cm_s[e] = 0.0;
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < nnz; j += stride) {
    const double v = (double)vals[j];
    const int64_t c = (int64_t)indices[j];
    atomicAdd(&cm_s[c], v);
    atomicAdd(&cm_s[d + c], v * v);
  }
  __syncthreads();
  for (int64_t e = threadIdx.x; e < 2 * d; e += 256)
    if (cm_s[e] != 0.0) atomicAdd(&out[e], cm_s[e]);
}

// ---------------------------------------------------------------------------
// fil_predict: forest inference (the reference's FIL predict kernel,
// tree.py:709-721 / cuML FIL). All trees live flattened in one node arena
// (per-tree root offsets); one THREAD walks every tree for its row,
// accumulating leaf values (class-count vote or regression mean). Routing
// rule is the training one: x < threshold goes LEFT.
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(256) void fil_predict_kernel(
    const float* __restrict__ X,        // [n, d]
    const int32_t* __restrict__ feat,   // arena [total_nodes]
    const float* __restrict__ thr,      // arena
    const int32_t* __restrict__ left,   // arena (tree-local ids)
    const int32_t* __restrict__ right,  // arena
    const float* __restrict__ value,    // arena [total_nodes, vw]
    const int64_t* __restrict__ roots,  // [T] arena offset of each tree root
    int64_t n, int d, int T, int vw, int classif,
    float* __restrict__ out) {          // [n, vw] summed votes / means
  const int64_t stride = (int64_t)gridDim.x * 256;
  float acc[16];  // vw <= 16 (host falls back to torch past that)
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const float* xrow = X + i * d;
    for (int c = 0; c < vw; ++c) acc[c] = 0.0f;
    for (int t = 0; t < T; ++t) {
      const int64_t base = roots[t];
      int node = 0;
      int f = feat[base + node];
      while (f >= 0) {
        node = (xrow[f] < thr[base + node]) ? left[base + node]
                                            : right[base + node];
        f = feat[base + node];
      }
      const float* v = value + (base + node) * vw;
      if (classif) {
        // normalized class-count vote (matches the torch traversal)
        float s = 0.0f;
        for (int c = 0; c < vw; ++c) s += v[c];
        s = fmaxf(s, 1e-12f);
        for (int c = 0; c < vw; ++c) acc[c] += v[c] / s;
      } else {
        acc[0] += v[0];  // (mean, count) leaves: mean is v[0]
      }
    }
    if (classif) {
      for (int c = 0; c < vw; ++c) out[i * vw + c] = acc[c];
    } else {
      out[i * vw + 0] = acc[0];
    }
  }
}

// ---------------------------------------------------------------------------
// softmax_residual_loss: per-row softmax (C>1) or sigmoid (C==1) residual
// and summed log-loss. resid = softmax(scores) - onehot(y) (or p - y).
// One wave per row chunk; memory-bound, fused to one pass.
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(256) void softmax_residual_kernel(
    const float* __restrict__ scores,  // [n, C]
    const int64_t* __restrict__ y,     // [n]
    int64_t n, int C,
    float* __restrict__ resid,         // [n, C]
    float* __restrict__ loss) {        // [1]
  const int64_t row0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  float local_loss = 0.0f;
  for (int64_t i = row0; i < n; i += stride) {
    const float* s = scores + i * C;
    float* r = resid + i * C;
    const int yi = (int)y[i];
    if (C == 1) {
      float z = s[0];
      float t = yi ? 1.0f : -1.0f;
      // log(1+exp(-t z)) stable
      float m = -t * z;
      local_loss += (m > 0 ? m : 0.0f) + __logf(1.0f + __expf(-fabsf(m)));
      float p = 1.0f / (1.0f + __expf(-z));
      r[0] = p - (float)yi;
    } else {
      float mx = s[0];
      for (int c = 1; c < C; ++c) mx = fmaxf(mx, s[c]);
      float denom = 0.0f;
      for (int c = 0; c < C; ++c) denom += __expf(s[c] - mx);
      float logd = __logf(denom);
      local_loss += -(s[yi] - mx - logd);
      for (int c = 0; c < C; ++c) {
        float p = __expf(s[c] - mx) / denom;
        r[c] = p - (c == yi ? 1.0f : 0.0f);
      }
    }
  }
  // block-reduce the loss, one atomic per wave
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    local_loss += __shfl_down(local_loss, off, 64);
  if ((threadIdx.x & 63) == 0) atomicAdd(loss, local_loss);
}

// ---------------------------------------------------------------------------
// host wrappers
// ---------------------------------------------------------------------------

static inline hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}


torch::Tensor dbscan_sweep(torch::Tensor X, torch::Tensor x_sq, int64_t row0,
                           int64_t n_rows, double eps2, int64_t mode,
                           torch::Tensor core, torch::Tensor labels,
                           torch::Tensor tile_idx, torch::Tensor tile_off) {
  TORCH_CHECK(X.is_cuda() && x_sq.is_cuda(), "device tensors required");
  TORCH_CHECK(X.dtype() == torch::kFloat32 && X.is_contiguous());
  const int64_t n = X.size(0);
  const int d = (int)X.size(1);
  auto out = torch::empty({n_rows}, X.options().dtype(torch::kInt32));
  if (n_rows == 0) return out;
  TORCH_CHECK(row0 >= 0 && row0 + n_rows <= n, "row slice out of range");
  if (mode == 1) {
    TORCH_CHECK(core.dtype() == torch::kUInt8 && core.is_contiguous());
    TORCH_CHECK(labels.dtype() == torch::kInt32 && labels.is_contiguous());
  }
  const int grid = (int)((n_rows + KM_BM - 1) / KM_BM);
  const bool pruned = tile_off.numel() > 0;
  if (pruned) {
    TORCH_CHECK(tile_idx.dtype() == torch::kInt32 && tile_idx.is_contiguous());
    TORCH_CHECK(tile_off.dtype() == torch::kInt32 && tile_off.is_contiguous());
    TORCH_CHECK(tile_off.numel() == grid + 1, "tile_off must have one entry per row block + 1");
  }
  hipLaunchKernelGGL(dbscan_sweep_kernel, dim3(grid), dim3(256), 0, cur_stream(),
                     X.data_ptr<float>(), x_sq.data_ptr<float>(), (int)n, d,
                     (int)row0, (int)n_rows, (float)eps2, (int)mode,
                     mode == 1 ? core.data_ptr<uint8_t>() : nullptr,
                     mode == 1 ? labels.data_ptr<int32_t>() : nullptr,
                     pruned ? tile_idx.data_ptr<int32_t>() : nullptr,
                     pruned ? tile_off.data_ptr<int32_t>() : nullptr,
                     out.data_ptr<int32_t>());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return out;
}


torch::Tensor umap_sgd(torch::Tensor emb, torch::Tensor tail_emb,
                       torch::Tensor heads, torch::Tensor tails,
                       torch::Tensor eps, int64_t n_epochs, double a, double b,
                       double lr, double repulsion, int64_t neg_rate,
                       bool move_tail, int64_t seed) {
  TORCH_CHECK(emb.is_cuda() && emb.dtype() == torch::kFloat32 && emb.is_contiguous());
  TORCH_CHECK(heads.dtype() == torch::kInt32 && tails.dtype() == torch::kInt32);
  TORCH_CHECK(eps.dtype() == torch::kFloat32);
  const int m = (int)heads.size(0);
  const int dim = (int)emb.size(1);
  const int n_vertices = (int)tail_emb.size(0);
  TORCH_CHECK(dim >= 1 && dim <= 4, "umap_sgd supports dim 1..4");
  auto next_due = eps.clone();
  const int grid = (m + 255) / 256;
  for (int epoch = 1; epoch <= (int)n_epochs; ++epoch) {
    const float alpha = (float)(lr * (1.0 - (double)epoch / (double)n_epochs));
#define UMAP_LAUNCH(D)                                                         \
    hipLaunchKernelGGL(umap_sgd_epoch_kernel<D>, dim3(grid), dim3(256), 0,     \
                       cur_stream(), emb.data_ptr<float>(),                    \
                       tail_emb.data_ptr<float>(), heads.data_ptr<int32_t>(),  \
                       tails.data_ptr<int32_t>(), eps.data_ptr<float>(),       \
                       next_due.data_ptr<float>(), m, n_vertices, (float)a,    \
                       (float)b, alpha, (float)repulsion, (int)neg_rate,       \
                       move_tail ? 1 : 0, epoch, (unsigned)(seed & 0xffffffff))
    switch (dim) {
      case 1: UMAP_LAUNCH(1); break;
      case 2: UMAP_LAUNCH(2); break;
      case 3: UMAP_LAUNCH(3); break;
      default: UMAP_LAUNCH(4); break;
    }
#undef UMAP_LAUNCH
    C10_HIP_KERNEL_LAUNCH_CHECK();
  }
  return emb;
}

std::vector<torch::Tensor> kmeans_assign(torch::Tensor X, torch::Tensor C,
                                         torch::Tensor x_sq) {
  TORCH_CHECK(X.is_cuda() && C.is_cuda() && x_sq.is_cuda(), "device tensors required");
  TORCH_CHECK(X.dtype() == torch::kFloat32 && C.dtype() == torch::kFloat32);
  TORCH_CHECK(X.is_contiguous() && C.is_contiguous());
  const int64_t n = X.size(0);
  const int d = (int)X.size(1);
  const int k_real = (int)C.size(0);
  auto c_sq = (C * C).sum(1);
  // Pad centers to a KM_BN multiple: a partial center tile routes BOTH the
  // X and C stages of that tile through the guarded per-element load path
  // (the de-pipelining trap in profiles/README.md) — at k=200 that is half
  // of all tiles and cost ~2x (209 ms vs ~100 ms on 100M x 128). Pad rows
  // carry c_sq = FLT_MAX so they can never win the argmin.
  const int k = (int)((k_real + KM_BN - 1) / KM_BN * KM_BN);
  if (k != k_real) {
    auto Cp = torch::zeros({(int64_t)k, (int64_t)d}, C.options());
    Cp.narrow(0, 0, k_real).copy_(C);
    auto cp = torch::full({(int64_t)k}, 3.0e38f, c_sq.options());
    cp.narrow(0, 0, k_real).copy_(c_sq);
    C = Cp.contiguous();
    c_sq = cp.contiguous();
  }
  auto labels = torch::empty({n}, X.options().dtype(torch::kInt32));
  auto min_dists = torch::empty({n}, X.options());
  auto inertia = torch::zeros({1}, X.options().dtype(torch::kFloat64));
  const int grid = (int)((n + KM_BM - 1) / KM_BM);
  if (n > 0) {
    // Register-staged BK=64 write-after-barrier is the one fused kernel: the
    // glds 2-/3-buffer and 256x256 variants lost or tied on MI355X
    // (1M x 3000, k=1000; profiles/README.md) and were removed.
    hipLaunchKernelGGL(kmeans_assign_kernel, dim3(grid), dim3(256), 0, cur_stream(),
                       X.data_ptr<float>(), C.data_ptr<float>(), x_sq.data_ptr<float>(),
                       c_sq.data_ptr<float>(), (int)n, d, k,
                       labels.data_ptr<int32_t>(), min_dists.data_ptr<float>(),
                       inertia.data_ptr<double>());
    C10_HIP_KERNEL_LAUNCH_CHECK();
  }
  return {labels, min_dists, inertia};
}

std::vector<torch::Tensor> label_accumulate(torch::Tensor X, torch::Tensor labels, int64_t k) {
  TORCH_CHECK(X.is_cuda() && labels.is_cuda());
  const int64_t n = X.size(0);
  const int d = (int)X.size(1);
  auto sums = torch::zeros({k, d}, X.options());
  auto counts = torch::zeros({k}, X.options());
  if (n == 0) return {sums, counts};
  const int64_t kd4 = k * (int64_t)d * 4;
  if (kd4 + k * 4 <= 120 * 1024 && labels.dtype() == torch::kInt32) {
    const unsigned grid = (unsigned)std::min<int64_t>(512, (n + 511) / 512 + 1);
    const int64_t rows_per_block = (n + grid - 1) / grid;
    const size_t lds = (size_t)kd4 + (size_t)k * 4;
    hipLaunchKernelGGL(label_accumulate_lds_kernel, dim3(grid), dim3(512), lds,
                       cur_stream(), X.data_ptr<float>(),
                       labels.data_ptr<int32_t>(), n, d, (int)k,
                       rows_per_block, sums.data_ptr<float>(),
                       counts.data_ptr<float>());
    C10_HIP_KERNEL_LAUNCH_CHECK();
    return {sums, counts};
  }
  {
    auto sorted = labels.to(torch::kInt64).sort();
    auto perm = std::get<1>(sorted).contiguous();
    auto sl = std::get<0>(sorted).contiguous();
    auto bounds = torch::arange(k + 1, labels.options().dtype(torch::kInt64));
    auto seg_off = torch::searchsorted(sl, bounds).contiguous();
    hipLaunchKernelGGL(segment_sum_kernel, dim3((unsigned)(k * LA_SPLIT)), dim3(256), 0,
                       cur_stream(), X.data_ptr<float>(), perm.data_ptr<int64_t>(),
                       seg_off.data_ptr<int64_t>(), d, sums.data_ptr<float>(),
                       counts.data_ptr<float>());
    C10_HIP_KERNEL_LAUNCH_CHECK();
  }
  return {sums, counts};
}

// (sums [k,d], counts [k], inertia f64 [1]) on the sorted segment path, k and
// the centres taken from C. `vec` selects the 16-byte row loads where the
// layout allows them.
std::vector<torch::Tensor> label_accumulate_inertia(torch::Tensor X, torch::Tensor labels,
                                                    torch::Tensor C, bool vec) {
  TORCH_CHECK(X.is_cuda() && labels.is_cuda() && C.is_cuda(), "device tensors required");
  TORCH_CHECK(X.dtype() == torch::kFloat32 && X.is_contiguous() && X.dim() == 2);
  TORCH_CHECK(C.dtype() == torch::kFloat32 && C.is_contiguous() && C.dim() == 2);
  TORCH_CHECK(C.size(1) == X.size(1), "X and C column counts disagree");
  TORCH_CHECK(labels.numel() == X.size(0), "one label per row");
  const int64_t n = X.size(0);
  const int64_t k = C.size(0);
  const int d = (int)X.size(1);
  auto sums = torch::zeros({k, d}, X.options());
  auto counts = torch::zeros({k}, X.options());
  auto inertia = torch::zeros({1}, X.options().dtype(torch::kFloat64));
  if (n == 0 || k == 0) return {sums, counts, inertia};
  auto sorted = labels.to(torch::kInt64).sort();
  auto perm = std::get<1>(sorted).contiguous();
  auto sl = std::get<0>(sorted).contiguous();
  auto bounds = torch::arange(k + 1, labels.options().dtype(torch::kInt64));
  auto seg_off = torch::searchsorted(sl, bounds).contiguous();
  const bool aligned = ((uintptr_t)X.data_ptr() | (uintptr_t)C.data_ptr()) % 16 == 0;
  if (vec && d % 4 == 0 && aligned)
    hipLaunchKernelGGL(segment_sum_inertia_kernel<true>, dim3((unsigned)(k * LA_SPLIT)),
                       dim3(256), 0, cur_stream(), X.data_ptr<float>(),
                       perm.data_ptr<int64_t>(), seg_off.data_ptr<int64_t>(),
                       C.data_ptr<float>(), d, sums.data_ptr<float>(),
                       counts.data_ptr<float>(), inertia.data_ptr<double>());
  else
    hipLaunchKernelGGL(segment_sum_inertia_kernel<false>, dim3((unsigned)(k * LA_SPLIT)),
                       dim3(256), 0, cur_stream(), X.data_ptr<float>(),
                       perm.data_ptr<int64_t>(), seg_off.data_ptr<int64_t>(),
                       C.data_ptr<float>(), d, sums.data_ptr<float>(),
                       counts.data_ptr<float>(), inertia.data_ptr<double>());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {sums, counts, inertia};
}

torch::Tensor gram_f32(torch::Tensor A) {
  TORCH_CHECK(A.is_cuda() && A.dtype() == torch::kFloat32 && A.is_contiguous());
  const int64_t n = A.size(0);
  const int d = (int)A.size(1);
  auto out = torch::zeros({d, d}, A.options());
  if (n > 0 && d > 0) {
    const int nb = (d + GR_BN - 1) / GR_BN;
    const int tri = nb * (nb + 1) / 2;
    int split = std::max(1, std::min(64, 768 / tri));
    dim3 grid((unsigned)(tri * split));
    hipLaunchKernelGGL(gram_kernel, grid, dim3(256), 0, cur_stream(),
                       A.data_ptr<float>(), n, d, nb, split, out.data_ptr<float>());
    C10_HIP_KERNEL_LAUNCH_CHECK();
    int mgrid = (int)std::min<int64_t>(2048, ((int64_t)d * d + 255) / 256);
    hipLaunchKernelGGL(gram_mirror_kernel, dim3(mgrid), dim3(256), 0, cur_stream(),
                       out.data_ptr<float>(), d);
    C10_HIP_KERNEL_LAUNCH_CHECK();
  }
  return out;
}

std::vector<torch::Tensor> knn_select(torch::Tensor Q, torch::Tensor I, int64_t k) {
  TORCH_CHECK(Q.is_cuda() && I.is_cuda());
  TORCH_CHECK(Q.dtype() == torch::kFloat32 && I.dtype() == torch::kFloat32);
  TORCH_CHECK(Q.is_contiguous() && I.is_contiguous());
  TORCH_CHECK(k >= 1 && k <= KN_KMAX, "knn_select supports k in [1, 64]");
  const int nq = (int)Q.size(0);
  const int ni = (int)I.size(0);
  const int d = (int)Q.size(1);
  auto q_sq = (Q * Q).sum(1);
  auto i_sq = (I * I).sum(1);
  const int qblocks = (nq + KN_QB - 1) / KN_QB;
  int isplit = std::max(1, std::min((ni + KN_IB - 1) / KN_IB, 512 / std::max(1, qblocks)));
  auto dist = torch::empty({nq, (int64_t)isplit, k}, Q.options());
  auto idx = torch::empty({nq, (int64_t)isplit, k}, Q.options().dtype(torch::kInt32));
  if (nq > 0 && ni > 0) {
    hipLaunchKernelGGL(knn_select_kernel, dim3((unsigned)(qblocks * isplit)), dim3(256),
                       0, cur_stream(), Q.data_ptr<float>(), I.data_ptr<float>(),
                       q_sq.data_ptr<float>(), i_sq.data_ptr<float>(), nq, ni, d,
                       (int)k, isplit, dist.data_ptr<float>(), idx.data_ptr<int32_t>());
    C10_HIP_KERNEL_LAUNCH_CHECK();
  }
  // merge partial top-k across item splits
  auto dflat = dist.view({nq, (int64_t)isplit * k});
  auto iflat = idx.view({nq, (int64_t)isplit * k});
  int64_t kk = std::min<int64_t>(k, (int64_t)isplit * k);
  auto top = dflat.topk(kk, /*dim=*/1, /*largest=*/false);
  auto vals = std::get<0>(top);
  auto order = std::get<1>(top);
  auto ids = iflat.gather(1, order);
  return {vals, ids.to(torch::kInt64)};
}

std::vector<torch::Tensor> softmax_residual_loss(torch::Tensor scores, torch::Tensor y) {
  TORCH_CHECK(scores.is_cuda() && y.is_cuda());
  TORCH_CHECK(scores.dtype() == torch::kFloat32);
  TORCH_CHECK(y.dtype() == torch::kInt64);
  const int64_t n = scores.size(0);
  const int C = scores.dim() > 1 ? (int)scores.size(1) : 1;
  auto resid = torch::empty_like(scores);
  auto loss = torch::zeros({1}, scores.options());
  if (n > 0) {
    int grid = (int)std::min<int64_t>(2048, (n + 255) / 256);
    hipLaunchKernelGGL(softmax_residual_kernel, dim3(grid), dim3(256), 0, cur_stream(),
                       scores.data_ptr<float>(), y.data_ptr<int64_t>(), n, C,
                       resid.data_ptr<float>(), loss.data_ptr<float>());
    C10_HIP_KERNEL_LAUNCH_CHECK();
  }
  return {resid, loss.squeeze(0)};
}

torch::Tensor rf_histogram(torch::Tensor Xb, torch::Tensor perm, torch::Tensor seg_off,
                           torch::Tensor feat_sel, torch::Tensor y, int64_t f0,
                           int64_t FC, int64_t n_bins, int64_t n_classes,
                           torch::Tensor sample, double y_max) {
  // Xb here is the COLUMN-major binned matrix [d, n_phys]
  TORCH_CHECK(Xb.is_cuda() && Xb.dtype() == torch::kUInt8 && Xb.is_contiguous());
  TORCH_CHECK(perm.dtype() == torch::kInt64 && seg_off.dtype() == torch::kInt64);
  const int d = (int)Xb.size(0);
  const int64_t n_phys = Xb.size(1);
  const int B = (int)seg_off.size(0) - 1;
  const bool classif = n_classes > 0;
  const int C = classif ? (int)n_classes : 2;
  const int mf = feat_sel.numel() > 0 ? (int)feat_sel.size(1) : 0;
  const bool has_sample = sample.numel() > 0;
  if (has_sample) TORCH_CHECK(sample.dtype() == torch::kInt32 && sample.is_contiguous());
  // regression packed-u64 path: caller supplies max|y| (computed once per
  // forest fit — a per-call .item() would sync every chunk) and the
  // per-node row-count cap gates it
  float y_scale = 0.0f, y_inv_scale = 0.0f;
  if (!classif && y_max > 0.0) {
    const int64_t vn = has_sample ? sample.numel() : perm.numel();
    if (vn < (1ll << 23)) {
      y_scale = (float)y_max;
      y_inv_scale = 1.0f / y_scale;
    }
  }
  const size_t lds = ((size_t)FC * n_bins * C + 1 & ~1ull) * 4 + (size_t)FC * 8;  // hist + col offsets
  TORCH_CHECK(lds <= 160 * 1024, "feature chunk too large for LDS");
  int split = std::max(1, (int)(1024 / std::max(1, B)));
  // split==1 writes every cell exactly once -> skip the zero-fill kernel
  auto out = split > 1
      ? torch::zeros({(int64_t)B, FC, n_bins, (int64_t)C}, Xb.options().dtype(torch::kFloat32))
      : torch::empty({(int64_t)B, FC, n_bins, (int64_t)C}, Xb.options().dtype(torch::kFloat32));
  hipLaunchKernelGGL(rf_histogram_kernel, dim3((unsigned)(B * split)), dim3(256), lds,
                     cur_stream(), Xb.data_ptr<uint8_t>(), perm.data_ptr<int64_t>(),
                     seg_off.data_ptr<int64_t>(),
                     mf > 0 ? feat_sel.data_ptr<int32_t>() : nullptr,
                     classif ? y.data_ptr<int32_t>() : nullptr,
                     classif ? nullptr : y.data_ptr<float>(),
                     has_sample ? sample.data_ptr<int32_t>() : nullptr, n_phys,
                     d, mf, (int)f0, (int)FC, (int)n_bins, C, split,
                     y_inv_scale, y_scale,
                     out.data_ptr<float>());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return out;
}

torch::Tensor rf_histogram_fw(torch::Tensor Xrm, torch::Tensor perm, torch::Tensor seg_off,
                              torch::Tensor feat_sel, torch::Tensor y, int64_t f0,
                              int64_t FC, int64_t n_bins, int64_t n_classes,
                              torch::Tensor sample, double y_max) {
  // Xrm is ROW-major [n_phys, d]
  TORCH_CHECK(Xrm.is_cuda() && Xrm.dtype() == torch::kUInt8 && Xrm.is_contiguous());
  TORCH_CHECK(perm.dtype() == torch::kInt64 && seg_off.dtype() == torch::kInt64);
  TORCH_CHECK(FC <= 32, "rf_histogram_fw: FC <= 32 (one lane group)");
  const int d = (int)Xrm.size(1);
  const int64_t n_phys = Xrm.size(0);
  const int B = (int)seg_off.size(0) - 1;
  const bool classif = n_classes > 0;
  const int C = classif ? (int)n_classes : 2;
  const int mf = feat_sel.numel() > 0 ? (int)feat_sel.size(1) : 0;
  const bool has_sample = sample.numel() > 0;
  float y_scale = 0.0f, y_inv_scale = 0.0f;
  if (!classif && y_max > 0.0) {
    const int64_t vn = has_sample ? sample.numel() : perm.numel();
    if (vn < (1ll << 23)) {
      y_scale = (float)y_max;
      y_inv_scale = 1.0f / y_scale;
    }
  }
  const size_t lds = (((size_t)FC * n_bins * C + 1) & ~1ull) * 4 + (size_t)FC * 4;
  TORCH_CHECK(lds <= 160 * 1024, "feature chunk too large for LDS");
  int split = std::max(1, (int)(1024 / std::max(1, B)));
  auto out = split > 1
      ? torch::zeros({(int64_t)B, FC, n_bins, (int64_t)C}, Xrm.options().dtype(torch::kFloat32))
      : torch::empty({(int64_t)B, FC, n_bins, (int64_t)C}, Xrm.options().dtype(torch::kFloat32));
  hipLaunchKernelGGL(rf_histogram_fw_kernel, dim3((unsigned)(B * split)), dim3(256), lds,
                     cur_stream(), Xrm.data_ptr<uint8_t>(), perm.data_ptr<int64_t>(),
                     seg_off.data_ptr<int64_t>(),
                     mf > 0 ? feat_sel.data_ptr<int32_t>() : nullptr,
                     classif ? y.data_ptr<int32_t>() : nullptr,
                     classif ? nullptr : y.data_ptr<float>(),
                     has_sample ? sample.data_ptr<int32_t>() : nullptr, n_phys,
                     d, mf, (int)f0, (int)FC, (int)n_bins, C, split,
                     y_inv_scale, y_scale,
                     out.data_ptr<float>());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return out;
}

std::vector<torch::Tensor> rf_best_split(torch::Tensor H, int64_t min_leaf,
                                          bool classif) {
  TORCH_CHECK(H.is_cuda() && H.dtype() == torch::kFloat32 && H.is_contiguous());
  const int B = (int)H.size(0);
  const int F = (int)H.size(1);
  const int nb = (int)H.size(2);
  const int C = (int)H.size(3);
  TORCH_CHECK(C <= RS_CMAX, "rf_best_split supports C <= 16");
  TORCH_CHECK(F < 0xffff && nb < 0xffff);
  auto gain = torch::empty({B}, H.options());
  auto feat = torch::empty({B}, H.options().dtype(torch::kInt32));
  auto bin = torch::empty({B}, H.options().dtype(torch::kInt32));
  auto lval = torch::empty({B, C}, H.options());
  auto rval = torch::empty({B, C}, H.options());
  if (B > 0) {
    hipLaunchKernelGGL(rf_best_split_kernel, dim3((unsigned)B), dim3(256), 0,
                       cur_stream(), H.data_ptr<float>(), F, nb, C,
                       (int)min_leaf, classif ? 1 : 0, gain.data_ptr<float>(),
                       feat.data_ptr<int32_t>(), bin.data_ptr<int32_t>(),
                       lval.data_ptr<float>(), rval.data_ptr<float>());
    C10_HIP_KERNEL_LAUNCH_CHECK();
  }
  return {gain, feat, bin, lval, rval};
}

std::vector<torch::Tensor> kmeans_argmin_kn(torch::Tensor dots, torch::Tensor x_sq,
                                            torch::Tensor c_sq) {
  TORCH_CHECK(dots.is_cuda() && dots.dtype() == torch::kFloat32 && dots.is_contiguous());
  TORCH_CHECK(x_sq.is_contiguous() && c_sq.is_contiguous());
  const int k = (int)dots.size(0);
  const int64_t n = dots.size(1);
  TORCH_CHECK((size_t)k * 4 <= 64 * 1024, "k too large for LDS stage");
  auto labels = torch::empty({n}, dots.options().dtype(torch::kInt32));
  auto min_d = torch::empty({n}, dots.options());
  auto inertia = torch::zeros({1}, dots.options().dtype(torch::kFloat64));
  const unsigned grid = (unsigned)std::min<int64_t>(4096, (n + 255) / 256 + 1);
  hipLaunchKernelGGL(kmeans_argmin_kn_kernel, dim3(grid), dim3(256), (size_t)k * 4,
                     cur_stream(), dots.data_ptr<float>(), x_sq.data_ptr<float>(),
                     c_sq.data_ptr<float>(), n, k, labels.data_ptr<int32_t>(),
                     min_d.data_ptr<float>(), inertia.data_ptr<double>());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {labels, min_d, inertia};
}

std::vector<torch::Tensor> kmeans_argmin_nk(torch::Tensor dots, torch::Tensor x_sq,
                                            torch::Tensor c_sq) {
  TORCH_CHECK(dots.is_cuda() && dots.dtype() == torch::kFloat32 && dots.is_contiguous());
  TORCH_CHECK(x_sq.is_contiguous() && c_sq.is_contiguous());
  const int64_t m = dots.size(0);
  const int k = (int)dots.size(1);
  auto labels = torch::empty({m}, dots.options().dtype(torch::kInt32));
  auto min_d = torch::empty({m}, dots.options());
  auto inertia = torch::zeros({1}, dots.options().dtype(torch::kFloat64));
  if (m > 0) {
    const unsigned grid = (unsigned)std::min<int64_t>(16384, (m + 3) / 4);
    hipLaunchKernelGGL(kmeans_argmin_nk_kernel, dim3(grid), dim3(256), 0,
                       cur_stream(), dots.data_ptr<float>(), x_sq.data_ptr<float>(),
                       c_sq.data_ptr<float>(), m, k, labels.data_ptr<int32_t>(),
                       min_d.data_ptr<float>(), inertia.data_ptr<double>());
    C10_HIP_KERNEL_LAUNCH_CHECK();
  }
  return {labels, min_d, inertia};
}

template <bool LO>
static std::vector<torch::Tensor> kmeans_split_impl(torch::Tensor A, torch::Tensor mu) {
  TORCH_CHECK(A.is_cuda() && A.dtype() == torch::kFloat32 && A.is_contiguous());
  TORCH_CHECK(mu.is_cuda() && mu.dtype() == torch::kFloat32 && mu.is_contiguous());
  TORCH_CHECK(A.dim() == 2 && mu.numel() == A.size(1), "mu must have one entry per column");
  const int64_t m = A.size(0);
  const int d = (int)A.size(1);
  const int dp = (d + 31) / 32 * 32;
  auto S = torch::empty({m, (int64_t)(LO ? 2 : 1) * dp}, A.options().dtype(torch::kBFloat16));
  auto a_sq = torch::empty({m}, A.options());
  if (m > 0) {
    const unsigned grid = (unsigned)std::min<int64_t>(1 << 20, (m + 3) / 4);
    auto* Sp = reinterpret_cast<uint16_t*>(S.data_ptr());
    const bool aligned = ((uintptr_t)A.data_ptr() | (uintptr_t)mu.data_ptr()) % 16 == 0;
    if (d % 4 == 0 && aligned)
      hipLaunchKernelGGL((kmeans_split_bf16_kernel<true, LO>), dim3(grid), dim3(256), 0,
                         cur_stream(), A.data_ptr<float>(), mu.data_ptr<float>(), m, d,
                         dp, Sp, a_sq.data_ptr<float>());
    else
      hipLaunchKernelGGL((kmeans_split_bf16_kernel<false, LO>), dim3(grid), dim3(256), 0,
                         cur_stream(), A.data_ptr<float>(), mu.data_ptr<float>(), m, d,
                         dp, Sp, a_sq.data_ptr<float>());
    C10_HIP_KERNEL_LAUNCH_CHECK();
  }
  return {S, a_sq};
}

std::vector<torch::Tensor> kmeans_split_bf16(torch::Tensor A, torch::Tensor mu) {
  return kmeans_split_impl<true>(A, mu);
}

// (H [m, dp] bf16, a_sq [m]): the hi half and the a_sq of kmeans_split_bf16,
// bit for bit, without the lo half.
std::vector<torch::Tensor> kmeans_split_bf16_hi(torch::Tensor A, torch::Tensor mu) {
  return kmeans_split_impl<false>(A, mu);
}

std::vector<torch::Tensor> kmeans_argmin_kn_screen(torch::Tensor dots, torch::Tensor a_sq,
                                                   torch::Tensor c_sq,
                                                   torch::Tensor margin_scale) {
  TORCH_CHECK(dots.is_cuda() && dots.dtype() == torch::kFloat32 && dots.is_contiguous());
  TORCH_CHECK(a_sq.is_cuda() && a_sq.dtype() == torch::kFloat32 && a_sq.is_contiguous());
  TORCH_CHECK(c_sq.is_cuda() && c_sq.dtype() == torch::kFloat32 && c_sq.is_contiguous());
  TORCH_CHECK(margin_scale.is_cuda() && margin_scale.dtype() == torch::kFloat32 &&
              margin_scale.numel() == 1);
  const int k = (int)dots.size(0);
  const int64_t m = dots.size(1);
  TORCH_CHECK(a_sq.numel() == m && c_sq.numel() == k, "a_sq / c_sq do not match dots");
  TORCH_CHECK((size_t)k * 4 <= 64 * 1024, "k too large for LDS stage");
  TORCH_CHECK(m < (int64_t)1 << 31, "row chunk too large for int32 row ids");
  auto iopt = dots.options().dtype(torch::kInt32);
  auto labels = torch::empty({m}, iopt);
  auto min_d = torch::empty({m}, dots.options());
  auto inertia = torch::zeros({1}, dots.options().dtype(torch::kFloat64));
  auto flagged = torch::empty({m}, iopt);
  auto n_flagged = torch::zeros({1}, iopt);
  if (m > 0) {
    const unsigned grid = (unsigned)std::min<int64_t>(4096, (m + 255) / 256);
    hipLaunchKernelGGL(kmeans_argmin_kn_screen_kernel, dim3(grid), dim3(256),
                       (size_t)k * 4, cur_stream(), dots.data_ptr<float>(),
                       a_sq.data_ptr<float>(), c_sq.data_ptr<float>(),
                       margin_scale.data_ptr<float>(), m, k, labels.data_ptr<int32_t>(),
                       min_d.data_ptr<float>(), inertia.data_ptr<double>(),
                       flagged.data_ptr<int32_t>(), n_flagged.data_ptr<int32_t>());
    C10_HIP_KERNEL_LAUNCH_CHECK();
  }
  return {labels, min_d, inertia, flagged, n_flagged};
}

void kmeans_refine(torch::Tensor X, torch::Tensor C, torch::Tensor dots,
                   torch::Tensor c_sq, torch::Tensor a_sq, torch::Tensor margin_scale,
                   torch::Tensor flagged_rows, torch::Tensor n_flagged,
                   torch::Tensor labels, torch::Tensor min_d, torch::Tensor inertia) {
  TORCH_CHECK(X.is_cuda() && X.dtype() == torch::kFloat32 && X.is_contiguous());
  TORCH_CHECK(C.is_cuda() && C.dtype() == torch::kFloat32 && C.is_contiguous());
  TORCH_CHECK(dots.is_cuda() && dots.dtype() == torch::kFloat32 && dots.is_contiguous());
  TORCH_CHECK(c_sq.dtype() == torch::kFloat32 && c_sq.is_contiguous());
  TORCH_CHECK(a_sq.dtype() == torch::kFloat32 && a_sq.is_contiguous());
  TORCH_CHECK(margin_scale.dtype() == torch::kFloat32 && margin_scale.numel() == 1);
  TORCH_CHECK(flagged_rows.dtype() == torch::kInt32 && flagged_rows.is_contiguous());
  TORCH_CHECK(n_flagged.dtype() == torch::kInt32 && n_flagged.numel() == 1);
  TORCH_CHECK(labels.dtype() == torch::kInt32 && labels.is_contiguous());
  TORCH_CHECK(min_d.dtype() == torch::kFloat32 && min_d.is_contiguous());
  TORCH_CHECK(inertia.dtype() == torch::kFloat64 && inertia.numel() == 1);
  const int64_t m = X.size(0);
  const int d = (int)X.size(1);
  const int k = (int)C.size(0);
  TORCH_CHECK(C.size(1) == d && dots.size(0) == k && dots.size(1) == m,
              "X, C and dots shapes disagree");
  TORCH_CHECK(c_sq.numel() == k && a_sq.numel() == m && flagged_rows.numel() == m &&
              labels.numel() == m && min_d.numel() == m, "per-row / per-centre sizes disagree");
  if (m == 0) return;
  hipLaunchKernelGGL(kmeans_refine_kernel, dim3(1024), dim3(256), 0, cur_stream(),
                     X.data_ptr<float>(), C.data_ptr<float>(), dots.data_ptr<float>(),
                     c_sq.data_ptr<float>(), a_sq.data_ptr<float>(),
                     margin_scale.data_ptr<float>(), flagged_rows.data_ptr<int32_t>(),
                     n_flagged.data_ptr<int32_t>(), m, d, k, labels.data_ptr<int32_t>(),
                     min_d.data_ptr<float>(), inertia.data_ptr<double>());
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

std::vector<torch::Tensor> rf_partition(torch::Tensor node_of_row, torch::Tensor lut,
                                        int64_t B) {
  TORCH_CHECK(node_of_row.is_cuda() && node_of_row.dtype() == torch::kInt64 &&
              node_of_row.is_contiguous());
  TORCH_CHECK(lut.is_cuda() && lut.dtype() == torch::kInt64 && lut.is_contiguous());
  TORCH_CHECK(B >= 1 && B <= 16384, "node batch too large for LDS counts");
  const int64_t n = node_of_row.size(0);
  auto counts = torch::zeros({B}, node_of_row.options().dtype(torch::kInt32));
  const size_t lds1 = (size_t)B * 4;
  const unsigned grid = (unsigned)std::min<int64_t>(1024, (n + 255) / 256 + 1);
  hipLaunchKernelGGL(rf_node_count_kernel, dim3(grid), dim3(256), lds1, cur_stream(),
                     node_of_row.data_ptr<int64_t>(), lut.data_ptr<int64_t>(), n, (int)B,
                     counts.data_ptr<int32_t>());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  auto seg_off = torch::zeros({B + 1}, node_of_row.options().dtype(torch::kInt64));
  seg_off.narrow(0, 1, B).copy_(torch::cumsum(counts, 0));
  auto cursor = seg_off.narrow(0, 0, B).to(torch::kInt32).contiguous();
  auto perm = torch::empty({n}, node_of_row.options().dtype(torch::kInt64));
  const size_t lds2 = (size_t)B * 8;
  hipLaunchKernelGGL(rf_partition_scatter_kernel, dim3(grid), dim3(256), lds2, cur_stream(),
                     node_of_row.data_ptr<int64_t>(), lut.data_ptr<int64_t>(), n, (int)B,
                     cursor.data_ptr<int32_t>(), perm.data_ptr<int64_t>());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {perm, seg_off};
}

void rf_reroute(torch::Tensor node_of_row, torch::Tensor lut2, torch::Tensor sfeat,
                torch::Tensor sbin, torch::Tensor lchild, torch::Tensor rchild,
                torch::Tensor Xb, torch::Tensor sample) {
  TORCH_CHECK(node_of_row.is_cuda() && node_of_row.dtype() == torch::kInt64);
  TORCH_CHECK(lut2.dtype() == torch::kInt64 && sfeat.dtype() == torch::kInt32 &&
              sbin.dtype() == torch::kInt32 && lchild.dtype() == torch::kInt64 &&
              rchild.dtype() == torch::kInt64 && Xb.dtype() == torch::kUInt8);
  const int64_t vn = node_of_row.size(0);
  const int64_t n_phys = Xb.size(1);  // [d, n_phys] column-major
  const int64_t d = Xb.size(0);
  const bool has_sample = sample.numel() > 0;
  if (has_sample) TORCH_CHECK(sample.dtype() == torch::kInt32 && sample.is_contiguous());
  const unsigned grid = (unsigned)std::min<int64_t>(2048, (vn + 255) / 256 + 1);
  hipLaunchKernelGGL(rf_reroute_kernel, dim3(grid), dim3(256), 0, cur_stream(),
                     node_of_row.data_ptr<int64_t>(), lut2.data_ptr<int64_t>(),
                     sfeat.data_ptr<int32_t>(), sbin.data_ptr<int32_t>(),
                     lchild.data_ptr<int64_t>(), rchild.data_ptr<int64_t>(),
                     Xb.data_ptr<uint8_t>(),
                     has_sample ? sample.data_ptr<int32_t>() : nullptr, n_phys,
                     vn, d);
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

void knn_merge_topk(torch::Tensor G, torch::Tensor q_sq, torch::Tensor i_sq,
                    int64_t base, torch::Tensor best_d, torch::Tensor best_i) {
  TORCH_CHECK(G.is_cuda() && G.dtype() == torch::kFloat32 && G.is_contiguous());
  TORCH_CHECK(best_d.size(1) == 64 && best_i.size(1) == 64,
              "slot buffers must be [nq, 64]");
  TORCH_CHECK(best_d.is_contiguous() && best_i.is_contiguous());
  TORCH_CHECK(q_sq.is_contiguous() && i_sq.is_contiguous());
  const int64_t nq = G.size(0);
  const int64_t c = G.size(1);
  TORCH_CHECK(i_sq.size(0) == c && q_sq.size(0) == nq && best_d.size(0) == nq);
  hipLaunchKernelGGL(knn_merge_topk_kernel<false>, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0,
                     cur_stream(), G.data_ptr<float>(), q_sq.data_ptr<float>(),
                     i_sq.data_ptr<float>(), nq, c, base, best_d.data_ptr<float>(),
                     best_i.data_ptr<int64_t>());
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

void knn_merge_topk_keys(torch::Tensor G, int64_t base, torch::Tensor best_d,
                         torch::Tensor best_i) {
  TORCH_CHECK(G.is_cuda() && G.dtype() == torch::kFloat32 && G.is_contiguous() && G.dim() == 2);
  TORCH_CHECK(best_d.is_cuda() && best_d.dtype() == torch::kFloat32 && best_d.dim() == 2);
  TORCH_CHECK(best_i.is_cuda() && best_i.dtype() == torch::kInt64 && best_i.dim() == 2);
  TORCH_CHECK(best_d.size(1) == 64 && best_i.size(1) == 64,
              "slot buffers must be [nq, 64]");
  TORCH_CHECK(best_d.is_contiguous() && best_i.is_contiguous());
  const int64_t nq = G.size(0);
  const int64_t c = G.size(1);
  TORCH_CHECK(best_d.size(0) == nq && best_i.size(0) == nq);
  if (nq == 0 || c == 0) return;
  hipLaunchKernelGGL(knn_merge_topk_kernel<true>, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0,
                     cur_stream(), G.data_ptr<float>(), (const float*)nullptr,
                     (const float*)nullptr, nq, c, base, best_d.data_ptr<float>(),
                     best_i.data_ptr<int64_t>());
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

template <int OP>
static void pairwise_dist_launch(unsigned grid, const float* Q, const float* I, int64_t nq,
                                 int64_t c, int d, float p, int64_t n_it, float* out) {
  hipLaunchKernelGGL(pairwise_dist_kernel<OP>, dim3(grid), dim3(256), 0, cur_stream(), Q, I,
                     nq, c, d, p, n_it, out);
}

// op: 0 L1 (sum |q-x|), 1 Linf (max), 2 Lp (sum |q-x|^p, no root), 3 canberra,
// 4 hamming (mismatch count, not divided by d)
void pairwise_dist(torch::Tensor Q, torch::Tensor I, int64_t op, double p, torch::Tensor out) {
  TORCH_CHECK(Q.is_cuda() && Q.dtype() == torch::kFloat32 && Q.is_contiguous() && Q.dim() == 2);
  TORCH_CHECK(I.is_cuda() && I.dtype() == torch::kFloat32 && I.is_contiguous() && I.dim() == 2);
  TORCH_CHECK(out.is_cuda() && out.dtype() == torch::kFloat32 && out.is_contiguous() &&
              out.dim() == 2);
  const int64_t nq = Q.size(0);
  const int64_t c = I.size(0);
  TORCH_CHECK(Q.size(1) == I.size(1), "Q and I must have the same number of columns");
  TORCH_CHECK(Q.size(1) >= 1 && Q.size(1) < (int64_t(1) << 24),
              "pairwise_dist supports 1 <= d < 2^24");
  TORCH_CHECK(out.size(0) == nq && out.size(1) == c, "out must be [nq, c]");
  TORCH_CHECK(op >= PD_L1 && op <= PD_HAMMING, "unknown pairwise_dist op");
  TORCH_CHECK(op != PD_LP || (std::isfinite(p) && p > 0.0), "minkowski p must be finite and > 0");
  if (nq == 0 || c == 0) return;
  const int d = (int)Q.size(1);
  const int64_t n_qt = (nq + PD_BM - 1) / PD_BM;
  const int64_t n_it = (c + PD_BM - 1) / PD_BM;
  TORCH_CHECK(n_qt * n_it < (int64_t(1) << 31), "pairwise_dist block is too large");
  const unsigned grid = (unsigned)(n_qt * n_it);
  const float* q = Q.data_ptr<float>();
  const float* it = I.data_ptr<float>();
  float* o = out.data_ptr<float>();
  switch (op) {
    case PD_L1: pairwise_dist_launch<PD_L1>(grid, q, it, nq, c, d, (float)p, n_it, o); break;
    case PD_LINF: pairwise_dist_launch<PD_LINF>(grid, q, it, nq, c, d, (float)p, n_it, o); break;
    case PD_LP: pairwise_dist_launch<PD_LP>(grid, q, it, nq, c, d, (float)p, n_it, o); break;
    case PD_CANBERRA:
      pairwise_dist_launch<PD_CANBERRA>(grid, q, it, nq, c, d, (float)p, n_it, o);
      break;
    default: pairwise_dist_launch<PD_HAMMING>(grid, q, it, nq, c, d, (float)p, n_it, o); break;
  }
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

template <int OP>
static void csr_pairwise_launch(unsigned grid, size_t lds, const int64_t* q_indptr,
                                const int32_t* q_col, const float* q_val, const int64_t* colptr,
                                const int32_t* c_row, const float* c_val, const float* A,
                                const float* B, int64_t nq, int c, int d, float p, float* out) {
  hipLaunchKernelGGL(csr_pairwise_kernel<OP>, dim3(grid), dim3(256), lds, cur_stream(), q_indptr,
                     q_col, q_val, colptr, c_row, c_val, A, B, nq, c, d, p, out);
}

// op: 0 dot (A + B - 2 acc), 1 L1, 2 Lp (no root), 3 canberra, 4 hamming
// (mismatch count), 5 jaccard (distance). Queries in CSR, the item chunk in
// CSC with chunk-local rows; A [nq] and B [c] are the per-row constants.
void csr_pairwise(torch::Tensor q_indptr, torch::Tensor q_col, torch::Tensor q_val,
                  torch::Tensor colptr, torch::Tensor c_row, torch::Tensor c_val, torch::Tensor A,
                  torch::Tensor B, int64_t op, double p, torch::Tensor out) {
  const torch::Tensor* all[] = {&q_indptr, &q_col, &q_val, &colptr, &c_row, &c_val, &A, &B, &out};
  for (const torch::Tensor* t : all)
    TORCH_CHECK(t->is_cuda() && t->device() == out.device() && t->is_contiguous(),
                "csr_pairwise tensors must be contiguous and on one device");
  TORCH_CHECK(q_indptr.dtype() == torch::kInt64 && colptr.dtype() == torch::kInt64,
              "indptr and colptr must be int64");
  TORCH_CHECK(q_col.dtype() == torch::kInt32 && c_row.dtype() == torch::kInt32,
              "column and row indices must be int32");
  TORCH_CHECK(q_val.dtype() == torch::kFloat32 && c_val.dtype() == torch::kFloat32 &&
                  A.dtype() == torch::kFloat32 && B.dtype() == torch::kFloat32 &&
                  out.dtype() == torch::kFloat32,
              "values, A, B and out must be float32");
  TORCH_CHECK(q_indptr.dim() == 1 && q_indptr.size(0) >= 1 && colptr.dim() == 1 &&
              colptr.size(0) >= 1 && A.dim() == 1 && B.dim() == 1 && out.dim() == 2);
  const int64_t nq = q_indptr.size(0) - 1;
  const int64_t c = B.size(0);
  const int64_t d = colptr.size(0) - 1;
  TORCH_CHECK(A.size(0) == nq, "A must be [nq]");
  TORCH_CHECK(c <= CP_CHUNK, "csr_pairwise chunk is limited to ", CP_CHUNK, " items by LDS");
  TORCH_CHECK(out.size(0) == nq && out.size(1) == c, "out must be [nq, c]");
  TORCH_CHECK(d < (int64_t(1) << 31), "csr_pairwise supports d < 2^31");
  TORCH_CHECK(q_col.numel() == q_val.numel() && c_row.numel() == c_val.numel());
  TORCH_CHECK(c_row.numel() < (int64_t(1) << 31), "csr_pairwise chunk nnz must be < 2^31");
  TORCH_CHECK(op >= CP_DOT && op <= CP_JACCARD, "unknown csr_pairwise op");
  TORCH_CHECK(op != CP_LP || (std::isfinite(p) && p > 0.0), "minkowski p must be finite and > 0");
  if (nq == 0 || c == 0) return;
  TORCH_CHECK((nq + 3) / 4 < (int64_t(1) << 31), "csr_pairwise block is too large");
  const unsigned grid = (unsigned)((nq + 3) / 4);
  const size_t lds = (size_t)4 * (size_t)c * sizeof(float);
#define CP_ARGS                                                                                  \
  grid, lds, q_indptr.data_ptr<int64_t>(), q_col.data_ptr<int32_t>(), q_val.data_ptr<float>(),   \
      colptr.data_ptr<int64_t>(), c_row.data_ptr<int32_t>(), c_val.data_ptr<float>(),            \
      A.data_ptr<float>(), B.data_ptr<float>(), nq, (int)c, (int)d, (float)p,                    \
      out.data_ptr<float>()
  switch (op) {
    case CP_DOT: csr_pairwise_launch<CP_DOT>(CP_ARGS); break;
    case CP_L1: csr_pairwise_launch<CP_L1>(CP_ARGS); break;
    case CP_LP: csr_pairwise_launch<CP_LP>(CP_ARGS); break;
    case CP_CANBERRA: csr_pairwise_launch<CP_CANBERRA>(CP_ARGS); break;
    case CP_HAMMING: csr_pairwise_launch<CP_HAMMING>(CP_ARGS); break;
    default: csr_pairwise_launch<CP_JACCARD>(CP_ARGS); break;
  }
#undef CP_ARGS
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

torch::Tensor gather_dists(torch::Tensor A, torch::Tensor B, torch::Tensor cand) {
  TORCH_CHECK(A.is_cuda() && A.dtype() == torch::kFloat32 && A.is_contiguous());
  TORCH_CHECK(B.dtype() == torch::kFloat32 && B.is_contiguous());
  TORCH_CHECK(cand.dtype() == torch::kInt64 && cand.is_contiguous());
  const int64_t r = cand.size(0);
  const int64_t m = cand.size(1);
  const int d = (int)A.size(1);
  TORCH_CHECK((int)B.size(1) == d && A.size(0) == r);
  TORCH_CHECK(d <= GD_DMAX, "gather_dists supports d <= 2048");
  auto out = torch::empty({r, m}, A.options());
  if (r > 0 && m > 0) {
    hipLaunchKernelGGL(gather_dists_kernel, dim3((unsigned)((r + 3) / 4)), dim3(256), 0,
                       cur_stream(), A.data_ptr<float>(), B.data_ptr<float>(),
                       cand.data_ptr<int64_t>(), r, m, d, out.data_ptr<float>());
    C10_HIP_KERNEL_LAUNCH_CHECK();
  }
  return out;
}

template <int NSEG>
static void ivf_scan_topk_launch(int64_t mode, unsigned grid, const float* Q,
                                 const float* Xs, const int64_t* list_off,
                                 const int64_t* pair_q, const int64_t* pair_list,
                                 const int64_t* pair_out, int64_t P, int64_t nq,
                                 int64_t n, int64_t nlist, int64_t n_out, int d,
                                 int k, float* part_key, int64_t* part_pos) {
  if (mode == 0)
    hipLaunchKernelGGL((ivf_scan_topk_kernel<NSEG, 0>), dim3(grid), dim3(256), 0,
                       cur_stream(), Q, Xs, list_off, pair_q, pair_list, pair_out,
                       P, nq, n, nlist, n_out, d, k, part_key, part_pos);
  else
    hipLaunchKernelGGL((ivf_scan_topk_kernel<NSEG, 1>), dim3(grid), dim3(256), 0,
                       cur_stream(), Q, Xs, list_off, pair_q, pair_list, pair_out,
                       P, nq, n, nlist, n_out, d, k, part_key, part_pos);
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

std::vector<torch::Tensor> ivf_scan_topk(torch::Tensor Q, torch::Tensor Xs,
                                         torch::Tensor list_off, torch::Tensor pair_q,
                                         torch::Tensor pair_list, torch::Tensor pair_out,
                                         int64_t n_out, int64_t k, int64_t mode) {
  TORCH_CHECK(Q.is_cuda() && Q.dtype() == torch::kFloat32 && Q.is_contiguous());
  TORCH_CHECK(Xs.is_cuda() && Xs.dtype() == torch::kFloat32 && Xs.is_contiguous());
  TORCH_CHECK(Q.dim() == 2 && Xs.dim() == 2 && Q.size(1) == Xs.size(1));
  for (const torch::Tensor* t : {&list_off, &pair_q, &pair_list, &pair_out})
    TORCH_CHECK(t->is_cuda() && t->dtype() == torch::kInt64 && t->is_contiguous() &&
                t->dim() == 1);
  const int64_t P = pair_q.size(0);
  TORCH_CHECK(pair_list.size(0) == P && pair_out.size(0) == P);
  TORCH_CHECK(list_off.size(0) >= 1);
  TORCH_CHECK(k >= 1 && k <= 64, "ivf_scan_topk supports 1 <= k <= 64");
  TORCH_CHECK(mode == 0 || mode == 1, "mode must be 0 (L2) or 1 (dot)");
  TORCH_CHECK(n_out >= 0);
  const int d = (int)Q.size(1);
  TORCH_CHECK(d >= 1 && d <= GD_DMAX, "ivf_scan_topk supports d <= 2048");
  const int64_t nq = Q.size(0), n = Xs.size(0), nlist = list_off.size(0) - 1;
  auto part_key = torch::full({n_out, 64}, INFINITY, Q.options());
  auto part_pos = torch::full({n_out, 64}, (int64_t)-1,
                              Q.options().dtype(torch::kInt64));
  if (P > 0 && n_out > 0) {
    TORCH_CHECK((P + 3) / 4 <= 0x7fffffffLL, "too many (query, list) pairs");
    const unsigned grid = (unsigned)((P + 3) / 4);
    const int nseg = (d + 63) >> 6;
#define IVF_SCAN_ARGS                                                             \
  mode, grid, Q.data_ptr<float>(), Xs.data_ptr<float>(),                          \
      list_off.data_ptr<int64_t>(), pair_q.data_ptr<int64_t>(),                   \
      pair_list.data_ptr<int64_t>(), pair_out.data_ptr<int64_t>(), P, nq, n,      \
      nlist, n_out, d, (int)k, part_key.data_ptr<float>(),                        \
      part_pos.data_ptr<int64_t>()
    if (nseg <= 1) ivf_scan_topk_launch<1>(IVF_SCAN_ARGS);
    else if (nseg <= 2) ivf_scan_topk_launch<2>(IVF_SCAN_ARGS);
    else if (nseg <= 4) ivf_scan_topk_launch<4>(IVF_SCAN_ARGS);
    else if (nseg <= 8) ivf_scan_topk_launch<8>(IVF_SCAN_ARGS);
    else if (nseg <= 16) ivf_scan_topk_launch<16>(IVF_SCAN_ARGS);
    else ivf_scan_topk_launch<32>(IVF_SCAN_ARGS);
#undef IVF_SCAN_ARGS
  }
  return {part_key, part_pos};
}

template <int SLOTS>
static void ivfpq_scan_topk_launch(int64_t mode, unsigned grid, size_t lds, const float* Q,
                                   const float* C, const float* cb, const uint8_t* codes,
                                   const int64_t* list_off, const int64_t* pair_q,
                                   const int64_t* pair_list, const int64_t* pair_out,
                                   int64_t P, int64_t nq, int64_t n, int64_t nlist,
                                   int64_t n_out, int d, int M, int ncodes, int ds,
                                   int64_t stride, int vec4, int k_cand, float* part_key,
                                   int64_t* part_pos) {
  if (mode == 0)
    hipLaunchKernelGGL((ivfpq_scan_topk_kernel<SLOTS, 0>), dim3(grid), dim3(256), lds,
                       cur_stream(), Q, C, cb, codes, list_off, pair_q, pair_list,
                       pair_out, P, nq, n, nlist, n_out, d, M, ncodes, ds, stride, vec4,
                       k_cand, part_key, part_pos);
  else
    hipLaunchKernelGGL((ivfpq_scan_topk_kernel<SLOTS, 1>), dim3(grid), dim3(256), lds,
                       cur_stream(), Q, C, cb, codes, list_off, pair_q, pair_list,
                       pair_out, P, nq, n, nlist, n_out, d, M, ncodes, ds, stride, vec4,
                       k_cand, part_key, part_pos);
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

// (part_key [n_out, 64*SLOTS], part_pos [n_out, 64*SLOTS]) with SLOTS = 1, 2
// or 4 for k_cand <= 64, 128, 256. codes_s is [n, stride] with stride >= M:
// columns past M are padding and are never used as codes.
std::vector<torch::Tensor> ivfpq_scan_topk(torch::Tensor Q, torch::Tensor C,
                                           torch::Tensor codebooks, torch::Tensor codes_s,
                                           torch::Tensor list_off, torch::Tensor pair_q,
                                           torch::Tensor pair_list, torch::Tensor pair_out,
                                           int64_t n_out, int64_t k_cand, int64_t mode) {
  for (const torch::Tensor* t : {&Q, &C, &codebooks})
    TORCH_CHECK(t->is_cuda() && t->dtype() == torch::kFloat32 && t->is_contiguous(),
                "ivfpq_scan_topk: Q, C and codebooks must be contiguous f32 device tensors");
  TORCH_CHECK(codes_s.is_cuda() && codes_s.dtype() == torch::kUInt8 &&
                  codes_s.is_contiguous() && codes_s.dim() == 2,
              "ivfpq_scan_topk: codes must be a contiguous [n, M] u8 device tensor");
  TORCH_CHECK(Q.dim() == 2 && C.dim() == 2 && codebooks.dim() == 3);
  for (const torch::Tensor* t : {&list_off, &pair_q, &pair_list, &pair_out})
    TORCH_CHECK(t->is_cuda() && t->dtype() == torch::kInt64 && t->is_contiguous() &&
                t->dim() == 1);
  const int64_t P = pair_q.size(0);
  TORCH_CHECK(pair_list.size(0) == P && pair_out.size(0) == P,
              "ivfpq_scan_topk: pair arrays differ in length");
  TORCH_CHECK(list_off.size(0) >= 1);
  const int64_t nq = Q.size(0), d = Q.size(1), nlist = list_off.size(0) - 1;
  const int64_t M = codebooks.size(0), ncodes = codebooks.size(1), ds = codebooks.size(2);
  const int64_t n = codes_s.size(0), stride = codes_s.size(1);
  TORCH_CHECK(d >= 1 && M >= 1 && ds >= 1 && d == M * ds,
              "ivfpq_scan_topk: d must equal M * ds");
  TORCH_CHECK(C.size(0) == nlist && C.size(1) == d,
              "ivfpq_scan_topk: C must be [nlist, d]");
  TORCH_CHECK(stride >= M, "ivfpq_scan_topk: code rows are shorter than M");
  TORCH_CHECK(ncodes >= 1 && ncodes <= 256 && (ncodes & (ncodes - 1)) == 0,
              "ivfpq_scan_topk: ncodes must be a power of two <= 256");
  TORCH_CHECK(k_cand >= 1 && k_cand <= 256, "ivfpq_scan_topk supports 1 <= k_cand <= 256");
  TORCH_CHECK(mode == 0 || mode == 1, "mode must be 0 (L2) or 1 (dot)");
  TORCH_CHECK(n_out >= 0);
  const int slots = k_cand <= 64 ? 1 : (k_cand <= 128 ? 2 : 4);
  const int64_t lds = ivfpq_lds_bytes(M, ncodes, d, slots);
  TORCH_CHECK(lds <= PQ_LDS_BUDGET, "ivfpq_scan_topk: LUT + query + merge buffer need ",
              lds, " bytes of LDS, over the ", PQ_LDS_BUDGET, " byte budget");
  auto part_key = torch::full({n_out, 64 * slots}, INFINITY, Q.options());
  auto part_pos = torch::full({n_out, 64 * slots}, (int64_t)-1,
                              Q.options().dtype(torch::kInt64));
  if (P > 0 && n_out > 0) {
    TORCH_CHECK(P <= 0x7fffffffLL, "too many (query, list) pairs");
    const int vec4 = (stride % 4 == 0) && ((uintptr_t)codes_s.data_ptr() % 4 == 0);
    // the LUT build reads codebook rows as float4 when ds % 4 == 0
    TORCH_CHECK(ds % 4 != 0 || (uintptr_t)codebooks.data_ptr() % 16 == 0,
                "ivfpq_scan_topk: codebooks must be 16 B aligned");
#define IVFPQ_SCAN_ARGS                                                           \
  mode, (unsigned)P, (size_t)lds, Q.data_ptr<float>(), C.data_ptr<float>(),       \
      codebooks.data_ptr<float>(), codes_s.data_ptr<uint8_t>(),                   \
      list_off.data_ptr<int64_t>(), pair_q.data_ptr<int64_t>(),                   \
      pair_list.data_ptr<int64_t>(), pair_out.data_ptr<int64_t>(), P, nq, n,      \
      nlist, n_out, (int)d, (int)M, (int)ncodes, (int)ds, stride, vec4,           \
      (int)k_cand, part_key.data_ptr<float>(), part_pos.data_ptr<int64_t>()
    if (slots == 1) ivfpq_scan_topk_launch<1>(IVFPQ_SCAN_ARGS);
    else if (slots == 2) ivfpq_scan_topk_launch<2>(IVFPQ_SCAN_ARGS);
    else ivfpq_scan_topk_launch<4>(IVFPQ_SCAN_ARGS);
#undef IVFPQ_SCAN_ARGS
  }
  return {part_key, part_pos};
}

// (keys [nq, k] f32, ids [nq, k] i32, stats [nq, 3] i32) of the graph search
// specified above cagra_search_kernel. hash_bits = 0 sizes the visited filter
// here: at least 2*max(itopk + search_width*deg, ns) slots, doubled while the
// block stays under CG_LDS_TARGET and the table under what 2n ids need.
std::vector<torch::Tensor> cagra_search(torch::Tensor Q, torch::Tensor X, torch::Tensor G,
                                        torch::Tensor seeds, int64_t k, int64_t itopk,
                                        int64_t search_width, int64_t max_iterations,
                                        int64_t hash_bits) {
  for (const torch::Tensor* t : {&Q, &X})
    TORCH_CHECK(t->is_cuda() && t->dtype() == torch::kFloat32 && t->is_contiguous() &&
                    t->dim() == 2,
                "cagra_search: Q and X must be contiguous 2-d f32 device tensors");
  for (const torch::Tensor* t : {&G, &seeds})
    TORCH_CHECK(t->is_cuda() && t->dtype() == torch::kInt32 && t->is_contiguous() &&
                    t->dim() == 2,
                "cagra_search: G and seeds must be contiguous 2-d i32 device tensors");
  TORCH_CHECK(X.device() == Q.device() && G.device() == Q.device() &&
                  seeds.device() == Q.device(),
              "cagra_search: all tensors must be on one device");
  const int64_t nq = Q.size(0), d = Q.size(1), n = X.size(0);
  const int64_t deg = G.size(1), ns = seeds.size(1);
  TORCH_CHECK(X.size(1) == d, "cagra_search: Q and X differ in width");
  TORCH_CHECK(d >= 1 && d <= 2048, "cagra_search supports 1 <= d <= 2048");
  TORCH_CHECK(n >= 1 && n < (1LL << 31), "cagra_search supports 1 <= n < 2**31");
  TORCH_CHECK(G.size(0) == n, "cagra_search: G must have one row per item");
  TORCH_CHECK(deg >= 1 && deg <= 128, "cagra_search supports 1 <= deg <= 128");
  TORCH_CHECK(seeds.size(0) == nq, "cagra_search: seeds and Q differ in row count");
  // seeds share the candidate buffer and the filter with an iteration's
  // candidates, so they get the same cap as search_width * deg
  TORCH_CHECK(ns >= 1 && ns <= 2048, "cagra_search supports 1 <= seeds per query <= 2048");
  TORCH_CHECK(k >= 1 && k <= itopk && itopk <= 512,
              "cagra_search supports 1 <= k <= itopk <= 512");
  TORCH_CHECK(search_width >= 1 && search_width * deg <= 2048,
              "cagra_search supports search_width >= 1 with search_width * deg <= 2048");
  TORCH_CHECK(max_iterations >= 1, "cagra_search: max_iterations must be >= 1");
  const int64_t min_slots = cg_pow2_ceil(2 * std::max(itopk + search_width * deg, ns));
  int64_t slots;
  if (hash_bits == 0) {
    const int64_t cap = std::max(min_slots, cg_pow2_ceil(2 * n));
    slots = min_slots;
    while (slots * 2 <= cap &&
           cagra_lds_bytes(d, itopk, search_width, deg, ns, slots * 2) <= CG_LDS_TARGET)
      slots *= 2;
  } else {
    TORCH_CHECK(hash_bits >= 1 && hash_bits <= 24 && (1LL << hash_bits) >= min_slots,
                "cagra_search: hash_bits must be 0 or give at least ", min_slots,
                " slots (2 * max(itopk + search_width * deg, seeds per query))");
    slots = 1LL << hash_bits;
  }
  int bits = 0;
  while ((1LL << bits) < slots) ++bits;
  const int64_t lds = cagra_lds_bytes(d, itopk, search_width, deg, ns, slots);
  TORCH_CHECK(lds <= CG_LDS_BUDGET, "cagra_search: list + candidates + visited filter + query need ",
              lds, " bytes of LDS, over the ", CG_LDS_BUDGET, " byte budget");
  auto keys = torch::empty({nq, k}, Q.options());
  auto ids = torch::empty({nq, k}, Q.options().dtype(torch::kInt32));
  auto stats = torch::empty({nq, 3}, Q.options().dtype(torch::kInt32));
  if (nq > 0) {
    TORCH_CHECK(nq <= 0x7fffffffLL, "too many queries");
    const int vec = (d % 4 == 0) && ((uintptr_t)X.data_ptr() % 16 == 0);
    const int max_it = (int)std::min<int64_t>(max_iterations, 0x7fffffffLL);
    hipLaunchKernelGGL(cagra_search_kernel, dim3((unsigned)nq), dim3(256), (size_t)lds,
                       cur_stream(), Q.data_ptr<float>(), X.data_ptr<float>(),
                       G.data_ptr<int32_t>(), seeds.data_ptr<int32_t>(), (int)n, (int)d,
                       (int)deg, (int)ns, (int)k, (int)itopk, (int)search_width, max_it,
                       bits, vec, keys.data_ptr<float>(), ids.data_ptr<int32_t>(),
                       stats.data_ptr<int32_t>());
    C10_HIP_KERNEL_LAUNCH_CHECK();
  }
  return {keys, ids, stats};
}

// (P [n, D_out] i32, detour [n, D] i32) of the graph pruning specified above
// cagra_prune_kernel.
std::vector<torch::Tensor> cagra_prune(torch::Tensor G, int64_t D_out) {
  TORCH_CHECK(G.is_cuda() && G.dtype() == torch::kInt32 && G.is_contiguous() && G.dim() == 2,
              "cagra_prune: G must be a contiguous 2-d i32 device tensor");
  const int64_t n = G.size(0), D = G.size(1);
  TORCH_CHECK(n < (1LL << 31), "cagra_prune supports n < 2**31");
  TORCH_CHECK(D >= 1 && D <= CP_MAX_D, "cagra_prune supports 1 <= D <= 256");
  TORCH_CHECK(D_out >= 1 && D_out <= D, "cagra_prune supports 1 <= D_out <= D");
  auto P = torch::empty({n, D_out}, G.options());
  auto detour = torch::empty({n, D}, G.options());
  if (n > 0) {
    const int64_t p2 = cg_pow2_ceil(D);
    int bits = 0;
    while ((1LL << bits) < 2 * p2) ++bits;
    const size_t lds = (size_t)cagra_prune_lds_bytes(D);
    const unsigned grid = (unsigned)std::min<int64_t>(n, 1LL << 20);
#define CAGRA_PRUNE_LAUNCH(CH)                                                              \
  hipLaunchKernelGGL(cagra_prune_kernel<CH>, dim3(grid), dim3(64), lds, cur_stream(),       \
                     G.data_ptr<int32_t>(), (int)n, (int)D, (int)D_out, (int)p2, bits,      \
                     P.data_ptr<int32_t>(), detour.data_ptr<int32_t>())
    const int ch = (int)((D + 63) / 64);
    if (ch == 1) CAGRA_PRUNE_LAUNCH(1);
    else if (ch == 2) CAGRA_PRUNE_LAUNCH(2);
    else if (ch == 3) CAGRA_PRUNE_LAUNCH(3);
    else CAGRA_PRUNE_LAUNCH(4);
#undef CAGRA_PRUNE_LAUNCH
    C10_HIP_KERNEL_LAUNCH_CHECK();
  }
  return {P, detour};
}

torch::Tensor fil_predict(torch::Tensor X, torch::Tensor feat, torch::Tensor thr,
                          torch::Tensor left, torch::Tensor right, torch::Tensor value,
                          torch::Tensor roots, bool classif) {
  TORCH_CHECK(X.is_cuda() && X.dtype() == torch::kFloat32 && X.is_contiguous());
  TORCH_CHECK(feat.dtype() == torch::kInt32 && left.dtype() == torch::kInt32 &&
              right.dtype() == torch::kInt32 && thr.dtype() == torch::kFloat32 &&
              value.dtype() == torch::kFloat32 && roots.dtype() == torch::kInt64);
  const int64_t n = X.size(0);
  const int d = (int)X.size(1);
  const int T = (int)roots.size(0);
  const int vw = (int)value.size(1);
  TORCH_CHECK(vw <= 16, "fil_predict supports value width <= 16");
  auto out = torch::zeros({n, (int64_t)vw}, X.options());
  if (n > 0 && T > 0) {
    const unsigned grid = (unsigned)std::min<int64_t>(4096, (n + 255) / 256 + 1);
    hipLaunchKernelGGL(fil_predict_kernel, dim3(grid), dim3(256), 0, cur_stream(),
                       X.data_ptr<float>(), feat.data_ptr<int32_t>(),
                       thr.data_ptr<float>(), left.data_ptr<int32_t>(),
                       right.data_ptr<int32_t>(), value.data_ptr<float>(),
                       roots.data_ptr<int64_t>(), n, d, T, vw, classif ? 1 : 0,
                       out.data_ptr<float>());
    C10_HIP_KERNEL_LAUNCH_CHECK();
  }
  return out;
}

torch::Tensor csr_fwd(torch::Tensor indptr, torch::Tensor indices, torch::Tensor vals,
                      torch::Tensor WT) {
  TORCH_CHECK(vals.is_cuda() && vals.dtype() == torch::kFloat32);
  TORCH_CHECK(WT.dtype() == torch::kFloat32 && WT.is_contiguous());
  const int64_t n = indptr.size(0) - 1;
  const int C = (int)WT.size(1);
  TORCH_CHECK(C <= 32, "csr_fwd supports C <= 32");
  auto scores = torch::empty({n, (int64_t)C}, vals.options());
  const unsigned grid = (unsigned)std::min<int64_t>(4096, (n + 255) / 256 + 1);
  if (indptr.dtype() == torch::kInt32) {
    hipLaunchKernelGGL(csr_fwd_kernel<int32_t>, dim3(grid), dim3(256), 0, cur_stream(),
                       indptr.data_ptr<int32_t>(), indices.data_ptr<int32_t>(),
                       vals.data_ptr<float>(), WT.data_ptr<float>(), n, C,
                       scores.data_ptr<float>());
    C10_HIP_KERNEL_LAUNCH_CHECK();
  } else {
    hipLaunchKernelGGL(csr_fwd_kernel<int64_t>, dim3(grid), dim3(256), 0, cur_stream(),
                       indptr.data_ptr<int64_t>(), indices.data_ptr<int64_t>(),
                       vals.data_ptr<float>(), WT.data_ptr<float>(), n, C,
                       scores.data_ptr<float>());
    C10_HIP_KERNEL_LAUNCH_CHECK();
  }
  return scores;
}

torch::Tensor csr_grad(torch::Tensor indptr, torch::Tensor indices, torch::Tensor vals,
                       torch::Tensor resid, int64_t d) {
  TORCH_CHECK(vals.is_cuda() && vals.dtype() == torch::kFloat32);
  TORCH_CHECK(resid.dtype() == torch::kFloat32 && resid.is_contiguous());
  const int64_t n = indptr.size(0) - 1;
  const int C = (int)resid.size(1);
  TORCH_CHECK(C <= 32, "csr_grad supports C <= 32");
  auto grad = torch::zeros({(int64_t)C, d}, vals.options());
  const unsigned grid = (unsigned)std::min<int64_t>(4096, (n + 255) / 256 + 1);
  const int64_t cd = (int64_t)C * d;
  const int use_lds = (cd * 4 <= 120 * 1024) ? 1 : 0;
  const size_t lds = use_lds ? (size_t)cd * 4 : 0;
  if (indptr.dtype() == torch::kInt32) {
    hipLaunchKernelGGL(csr_grad_kernel<int32_t>, dim3(grid), dim3(256), lds, cur_stream(),
                       indptr.data_ptr<int32_t>(), indices.data_ptr<int32_t>(),
                       vals.data_ptr<float>(), resid.data_ptr<float>(), n, d, C, use_lds,
                       grad.data_ptr<float>());
    C10_HIP_KERNEL_LAUNCH_CHECK();
  } else {
    hipLaunchKernelGGL(csr_grad_kernel<int64_t>, dim3(grid), dim3(256), lds, cur_stream(),
                       indptr.data_ptr<int64_t>(), indices.data_ptr<int64_t>(),
                       vals.data_ptr<float>(), resid.data_ptr<float>(), n, d, C, use_lds,
                       grad.data_ptr<float>());
    C10_HIP_KERNEL_LAUNCH_CHECK();
  }
  return grad;
}

torch::Tensor csr_col_moments(torch::Tensor indices, torch::Tensor vals, int64_t d) {
  TORCH_CHECK(vals.is_cuda() && vals.dtype() == torch::kFloat32);
  TORCH_CHECK(d * 16 <= 160 * 1024, "csr_col_moments: d too large for LDS");
  const int64_t nnz = vals.size(0);
  auto out = torch::zeros({2, d}, vals.options().dtype(torch::kFloat64));
  const unsigned grid = (unsigned)std::min<int64_t>(2048, (nnz + 255) / 256 + 1);
  const size_t lds = (size_t)d * 16;
  if (indices.dtype() == torch::kInt32) {
    hipLaunchKernelGGL(csr_col_moments_kernel<int32_t>, dim3(grid), dim3(256), lds,
                       cur_stream(), indices.data_ptr<int32_t>(),
                       vals.data_ptr<float>(), nnz, d, out.data_ptr<double>());
    C10_HIP_KERNEL_LAUNCH_CHECK();
  } else {
    hipLaunchKernelGGL(csr_col_moments_kernel<int64_t>, dim3(grid), dim3(256), lds,
                       cur_stream(), indices.data_ptr<int64_t>(),
                       vals.data_ptr<float>(), nnz, d, out.data_ptr<double>());
    C10_HIP_KERNEL_LAUNCH_CHECK();
  }
  return out;
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("fil_predict", &fil_predict, "forest inference (FIL-style traversal)");
  m.def("csr_fwd", &csr_fwd, "CSR scores = A @ WT (thread per row)");
  m.def("csr_grad", &csr_grad, "CSR grad = (A^T R)^T by column scatter");
  m.def("csr_col_moments", &csr_col_moments, "per-column sum/sumsq of CSR values");
  m.def("kmeans_assign", &kmeans_assign, "fused MFMA distance + argmin");
  m.def("kmeans_argmin_kn", &kmeans_argmin_kn, "argmin epilogue over a [k,n] GEMM dot block");
  m.def("kmeans_argmin_nk", &kmeans_argmin_nk, "argmin epilogue over a row-major [m,k] GEMM dot block");
  m.def("kmeans_split_bf16", &kmeans_split_bf16, "centre + split f32 rows into bf16 hi|lo halves, with |x'|^2");
  m.def("kmeans_split_bf16_hi", &kmeans_split_bf16_hi, "centre + round f32 rows to their bf16 hi plane, with |x'|^2");
  m.def("kmeans_argmin_kn_screen", &kmeans_argmin_kn_screen, "best/second argmin over a screened [k,n] dot block; flags near-ties");
  m.def("kmeans_refine", &kmeans_refine, "exact f64 decision for the flagged rows");
  m.def("label_accumulate", &label_accumulate, "per-center sum/count scatter");
  m.def("label_accumulate_inertia", &label_accumulate_inertia, "sorted per-center sum/count + sum (x - c)^2 in the same pass",
        py::arg("X"), py::arg("labels"), py::arg("C"), py::arg("vec") = LA_VEC_DEFAULT);
  m.def("gram_f32", &gram_f32, "A^T A via MFMA f32");
  m.def("softmax_residual_loss", &softmax_residual_loss, "fused softmax residual + loss");
  m.def("knn_select", &knn_select, "fused MFMA distance + in-LDS top-k");
  m.def("rf_histogram", &rf_histogram, "LDS-privatized RF split histograms");
  m.def("rf_histogram_fw", &rf_histogram_fw, "feature-wide RF histograms (lanes over sorted features)");
  m.def("rf_best_split", &rf_best_split, "fused RF gain scan + block-best reduce");
  m.def("dbscan_sweep", &dbscan_sweep, "fused eps-neighborhood count / min-core-label pass");
  m.def("umap_sgd", &umap_sgd, "edge-sampled UMAP SGD (all epochs, Hogwild)");
  m.def("rf_partition", &rf_partition, "counting-sort rows by node -> (perm, seg_off)");
  m.def("rf_reroute", &rf_reroute, "one-pass row-to-child reassignment");
  m.def("knn_merge_topk", &knn_merge_topk, "running top-k merge over a GEMM dot block");
  m.def("knn_merge_topk_keys", &knn_merge_topk_keys,
        "running top-k merge over a block of distance keys");
  m.def("pairwise_dist", &pairwise_dist,
        "register-tiled all-pairs distance keys (L1, Linf, Lp, canberra, hamming)");
  m.def("csr_pairwise", &csr_pairwise,
        "[nq, c] distance keys of CSR queries against a CSC item chunk");
  m.def("gather_dists", &gather_dists, "gathered row-vs-candidates squared distances");
  m.def("ivf_scan_topk", &ivf_scan_topk, "fused IVF-Flat probed-list scan + running top-k");
  m.def("ivfpq_scan_topk", &ivfpq_scan_topk,
        "fused IVF-PQ ADC scan: in-LDS lookup table + per-pair top-k_cand");
  m.def("cagra_search", &cagra_search,
        "fused graph beam search: in-LDS itopk list, visited filter and merge per query",
        py::arg("Q"), py::arg("X"), py::arg("G"), py::arg("seeds"), py::arg("k"),
        py::arg("itopk"), py::arg("search_width"), py::arg("max_iterations"),
        py::arg("hash_bits") = 0);
  m.def("cagra_prune", &cagra_prune,
        "rank-based detour counts of a kNN graph and its rows reordered by them",
        py::arg("G"), py::arg("D_out"));
  m.attr("_is_hip") = true;
}
