// Embedding projections of the reference's visualize.py on the device: PCA (column means, centred Gram matrix,
// projection - the D x D eigenproblem is the host's, numpy.linalg.eigh in fp64) and exact t-SNE as scikit-learn's
// TSNE(method="exact") states it: pairwise squared distances, _binary_search_perplexity, _joint_probabilities,
// _kl_divergence and _gradient_descent.  tests/tsne_oracle.py states the same in numpy fp64.
//
// Every reduction is a fixed-order sum of partials (wave butterfly, then the waves, blocks and column splits in index
// order): no floating-point atomics, two calls on one input return the same bits.  Terms and sums are fp64 - the vector
// fp64 rate of this part equals its unpacked fp32 rate, and the O(N^2) passes are bound by their fp32 operand (P, x),
// not by the arithmetic - and every fp32 output is rounded once.
//
// The O(N^2) passes of the descent (tsne_z_kernel, tsne_pair_kernel, tsne_kl_kernel) give a thread one ROW i and walk
// the columns j of a column split, reading P[j][i]: the joint P is symmetric to the bit (tsne_joint_kernel makes it so),
// so lane i reads its own p_ij while the wave's 64 reads are consecutive addresses, y_j is a broadcast from LDS, and a
// row's sum needs no cross-lane step.  N / 256 row tiles alone leave most compute units idle at N = 10^4, so the columns
// are split as well (kPairBlocks blocks in all) and tsne_update_kernel adds a row's split partials in split order.
//
// An iteration is two passes over the pairs: Z = sum n_ij first (the embedding alone: no memory traffic to speak of),
// then the gradient with scikit-learn's own terms (p_ij - max(n_ij / Z, eps)) n_ij (y_i - y_j) while P streams by once.
// The one-pass form 4 (attr - rep / Z) cannot apply the floor of q, and it loses the exact cancellation of p and q
// (N = 2, or any converged pair) to the rounding of two separately accumulated sums; DESIGN.md has the cost.
//
// The schedule never needs the host: a 64-byte status record in device memory carries "stopped", the best error and the
// iteration it was seen at; tsne_check_kernel applies _gradient_descent's stop rules to it, and every kernel of a later
// iteration returns at once when it says stopped.
#include "air_common.h"

#include <cfloat>
#include <cmath>

namespace {

constexpr int kVisMaxN = 16384;
constexpr int kVisMaxD = 1024;
constexpr int kPcaMaxK = 16;
constexpr int kThreads = 256;
constexpr double kEps = 2.220446049250313e-16;  // MACHINE_EPSILON of _t_sne.py: np.finfo(np.double).eps

// ---- fixed-order block sums (256 threads): butterfly inside the wave (every lane ends with the same bits), then the
// four waves in index order
__device__ __forceinline__ double block_sum_d(double v, double* sh) {
  v = air_wave_sum_d(v);
  __syncthreads();  // (sh may still be read from a previous sum)
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = sh[0];
  for (int w = 1; w < kThreads / 64; ++w) s += sh[w];
  return s;
}
// sum of p[0 .. n) by one block: thread t takes p[t], p[t + 256], ... in that order
__device__ __forceinline__ double block_sum_array_d(const double* __restrict__ p, int n, double* sh) {
  double s = 0.0;
  for (int k = threadIdx.x; k < n; k += kThreads) s += p[k];
  return block_sum_d(s, sh);
}

// ------------------------------------------------------------------------------------------------ PCA
constexpr int kPcaRowChunks = 64;  // column-sum partials
constexpr int kGramTile = 64;
constexpr int kGramMaxSplit = 16;

struct PcaPlan {
  int chunks, rows_per_chunk;  // column sums
  int tiles, split, rows_per_split;
  size_t colsum_off, gram_off, bytes;
};

__host__ PcaPlan pca_plan(int N, int D) {
  PcaPlan p;
  p.chunks = (N + 63) / 64 < kPcaRowChunks ? (N + 63) / 64 : kPcaRowChunks;
  p.rows_per_chunk = (N + p.chunks - 1) / p.chunks;
  p.tiles = (D + kGramTile - 1) / kGramTile;
  const int pairs = p.tiles * (p.tiles + 1) / 2;
  int split = (512 + pairs - 1) / pairs;
  const int by_rows = (N + 63) / 64;
  if (split > by_rows) split = by_rows;
  if (split > kGramMaxSplit) split = kGramMaxSplit;
  if (split < 1) split = 1;
  p.rows_per_split = ((N + split - 1) / split + 15) / 16 * 16;
  p.split = (N + p.rows_per_split - 1) / p.rows_per_split;
  p.colsum_off = 0;
  p.gram_off = (size_t)kPcaRowChunks * kVisMaxD * sizeof(double);
  p.bytes = p.gram_off + (size_t)p.split * D * D * sizeof(double);
  return p;
}

__global__ __launch_bounds__(kThreads) void pca_colsum_kernel(const float* __restrict__ x, int N, int D, int rows_per_chunk,
                                                              double* __restrict__ partial) {
  const int d = blockIdx.x * kThreads + threadIdx.x;
  if (d >= D) return;
  const int n0 = blockIdx.y * rows_per_chunk;
  const int n1 = n0 + rows_per_chunk < N ? n0 + rows_per_chunk : N;
  double s = 0.0;
  for (int n = n0; n < n1; ++n) s += (double)x[(size_t)n * D + d];
  partial[(size_t)blockIdx.y * D + d] = s;
}

__global__ __launch_bounds__(kThreads) void pca_mean_kernel(const double* __restrict__ partial, int N, int D, int chunks,
                                                            float* __restrict__ mean) {
  const int d = blockIdx.x * kThreads + threadIdx.x;
  if (d >= D) return;
  double s = 0.0;
  for (int c = 0; c < chunks; ++c) s += partial[(size_t)c * D + d];
  mean[d] = (float)(s / (double)N);
}

// Centred Gram tile (ti <= tj) of one row split: G[a][b] = sum_n (x[n][a] - mean[a]) * (x[n][b] - mean[b]), the
// differences in fp32 (as numpy centres an fp32 matrix), products and sums in fp64, rows in index order.
__global__ __launch_bounds__(kThreads) void pca_gram_kernel(const float* __restrict__ x, const float* __restrict__ mean, int N,
                                                            int D, int rows_per_split, double* __restrict__ partial) {
  const int ti = blockIdx.x, tj = blockIdx.y;
  if (tj < ti) return;
  __shared__ float As[16][kGramTile + 4];
  __shared__ float Bs[16][kGramTile + 4];
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
  const int lr = t >> 4, lc = (t & 15) * 4;  // staging: row lr of the 16, columns lc .. lc + 3
  const int n0 = blockIdx.z * rows_per_split;
  const int n1 = n0 + rows_per_split < N ? n0 + rows_per_split : N;
  double acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
  float ma[4], mb[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int ca = ti * kGramTile + lc + q, cb = tj * kGramTile + lc + q;
    ma[q] = ca < D ? mean[ca] : 0.0f;
    mb[q] = cb < D ? mean[cb] : 0.0f;
  }
  for (int nb = n0; nb < n1; nb += 16) {
    const int n = nb + lr;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int ca = ti * kGramTile + lc + q, cb = tj * kGramTile + lc + q;
      As[lr][lc + q] = (n < n1 && ca < D) ? x[(size_t)n * D + ca] - ma[q] : 0.0f;
      Bs[lr][lc + q] = (n < n1 && cb < D) ? x[(size_t)n * D + cb] - mb[q] : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      double a[4], b[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        a[q] = (double)As[r][ty * 4 + q];
        b[q] = (double)Bs[r][tx * 4 + q];
      }
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[p][q] = fma(a[p], b[q], acc[p][q]);
    }
    __syncthreads();
  }
  double* out = partial + (size_t)blockIdx.z * D * D;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int a = ti * kGramTile + ty * 4 + p;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int b = tj * kGramTile + tx * 4 + q;
      if (a < D && b < D) out[(size_t)a * D + b] = acc[p][q];
    }
  }
}

// gram[a][b] = sum over the row splits, in split order, of the upper tile's entry: both halves carry the same bits
__global__ __launch_bounds__(kThreads) void pca_gram_reduce_kernel(const double* __restrict__ partial, int D, int split,
                                                                   double* __restrict__ gram) {
  const size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= (size_t)D * D) return;
  const int a = (int)(e / D), b = (int)(e % D);
  const bool upper = a / kGramTile <= b / kGramTile;
  const size_t src = upper ? (size_t)a * D + b : (size_t)b * D + a;
  double s = 0.0;
  for (int k = 0; k < split; ++k) s += partial[(size_t)k * D * D + src];
  gram[e] = s;
}

// out[n][c] = sum_d (x[n][d] - mean[d]) * comps[c][d]: one wave per row, lane l takes d = l, l + 64, ...
__global__ __launch_bounds__(kThreads) void pca_project_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                               const float* __restrict__ comps, int N, int D, int K,
                                                               float* __restrict__ out) {
  const int n = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (n >= N) return;  // (wave-uniform)
  const int lane = threadIdx.x & 63;
  for (int c = 0; c < K; ++c) {
    double s = 0.0;
    for (int d = lane; d < D; d += 64) s = fma((double)(x[(size_t)n * D + d] - mean[d]), (double)comps[(size_t)c * D + d], s);
    s = air_wave_sum_d(s);
    if (lane == 0) out[(size_t)n * K + c] = (float)s;
  }
}

// ------------------------------------------------------------------------------- pairwise squared distances
// 64 x 64 tile per block, 4 x 4 per thread, 16 features per LDS stage.  d[i][j] = sum_k (x_i[k] - x_j[k])^2 in feature
// order, differences (exact), squares and sums in fp64, rounded to fp32 once: (i, j) and (j, i) add the same squares in
// the same order - equal bits - and i == j or two equal rows add zeros.  Features beyond D are staged as 0 in both
// operands.
constexpr int kDistTile = 64;
constexpr int kDistK = 16;

template <bool VEC>
__global__ __launch_bounds__(kThreads) void sqdist_kernel(const float* __restrict__ x, int N, int D, float* __restrict__ out) {
  __shared__ float As[kDistK][kDistTile + 4];
  __shared__ float Bs[kDistK][kDistTile + 4];
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
  const int lr = t >> 2, lk = (t & 3) * 4;  // staging: row lr of the 64, features lk .. lk + 3 of the 16
  const int ra = blockIdx.y * kDistTile + lr, rb = blockIdx.x * kDistTile + lr;
  double acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
  for (int k0 = 0; k0 < D; k0 += kDistK) {
    float va[4], vb[4];
    const int k = k0 + lk;
    if (VEC) {  // D % 4 == 0 and x 16-byte aligned: k < D covers k + 3
      const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 a4 = (ra < N && k < D) ? *reinterpret_cast<const float4*>(x + (size_t)ra * D + k) : z;
      const float4 b4 = (rb < N && k < D) ? *reinterpret_cast<const float4*>(x + (size_t)rb * D + k) : z;
      va[0] = a4.x; va[1] = a4.y; va[2] = a4.z; va[3] = a4.w;
      vb[0] = b4.x; vb[1] = b4.y; vb[2] = b4.z; vb[3] = b4.w;
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        va[q] = (ra < N && k + q < D) ? x[(size_t)ra * D + k + q] : 0.0f;
        vb[q] = (rb < N && k + q < D) ? x[(size_t)rb * D + k + q] : 0.0f;
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      As[lk + q][lr] = va[q];
      Bs[lk + q][lr] = vb[q];
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < kDistK; ++kk) {
      double a[4], b[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        a[q] = (double)As[kk][ty * 4 + q];
        b[q] = (double)Bs[kk][tx * 4 + q];
      }
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const double diff = a[p] - b[q];
          acc[p][q] = fma(diff, diff, acc[p][q]);
        }
    }
    __syncthreads();
  }
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int i = blockIdx.y * kDistTile + ty * 4 + p;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = blockIdx.x * kDistTile + tx * 4 + q;
      if (i < N && j < N) out[(size_t)i * N + j] = (float)acc[p][q];
    }
  }
}

// ------------------------------------------------------------------------------- conditional affinities
// _binary_search_perplexity (sklearn/manifold/_utils.pyx) for one row per block, in its own fp64: beta from 1, doubled
// or halved while a bound is infinite, at most 100 steps, stop at |H - log(perplexity)| <= 1e-5 (the fp32 constant the
// .pyx declares), a zero row sum replaced by the fp32 constant 1e-8.  The row of distances is re-read from L2 per step;
// the cost is the fp64 exp.
__global__ __launch_bounds__(kThreads) void tsne_affinity_kernel(const float* __restrict__ dist, int N, double log_perp,
                                                                 float* __restrict__ cond, float* __restrict__ beta_out) {
  __shared__ double sh[kThreads / 64];
  const int i = blockIdx.x;
  const float* __restrict__ d = dist + (size_t)i * N;
  const double tol = (double)1e-5f, tiny = (double)1e-8f;
  double beta = 1.0, beta_min = -INFINITY, beta_max = INFINITY, sum = 1.0;
  for (int step = 0; step < 100; ++step) {
    double s = 0.0, sd = 0.0;
    for (int j = threadIdx.x; j < N; j += kThreads) {
      if (j == i) continue;
      const double dj = (double)d[j];
      const double e = exp(-dj * beta);
      s += e;
      sd = fma(dj, e, sd);
    }
    s = block_sum_d(s, sh);
    sd = block_sum_d(sd, sh);
    if (s == 0.0) s = tiny;
    sum = s;
    const double diff = log(s) + beta * (sd / s) - log_perp;  // (every thread holds the same bits: uniform branches)
    if (fabs(diff) <= tol) break;
    if (diff > 0.0) {
      beta_min = beta;
      beta = beta_max == INFINITY ? beta * 2.0 : (beta + beta_max) * 0.5;
    } else {
      beta_max = beta;
      beta = beta_min == -INFINITY ? beta * 0.5 : (beta + beta_min) * 0.5;
    }
    if (step == 99) beta = diff > 0.0 ? beta_min : beta_max;  // the row keeps the last step's beta, as the .pyx's P does
  }
  for (int j = threadIdx.x; j < N; j += kThreads)
    cond[(size_t)i * N + j] = j == i ? 0.0f : (float)(exp(-(double)d[j] * beta) / sum);
  if (threadIdx.x == 0) beta_out[i] = (float)beta;
}

// ------------------------------------------------------------------------------- joint distribution
__global__ __launch_bounds__(kThreads) void tsne_rowsum_kernel(const float* __restrict__ c, int N, double* __restrict__ rowsum) {
  __shared__ double sh[kThreads / 64];
  const int i = blockIdx.x;
  double s = 0.0;
  for (int j = threadIdx.x; j < N; j += kThreads) s += (double)c[(size_t)i * N + j];
  s = block_sum_d(s, sh);
  if (threadIdx.x == 0) rowsum[i] = s;
}

__global__ __launch_bounds__(kThreads) void tsne_total_kernel(const double* __restrict__ rowsum, int N, double* __restrict__ total) {
  __shared__ double sh[kThreads / 64];
  const double s = block_sum_array_d(rowsum, N, sh);
  if (threadIdx.x == 0) total[0] = fmax(2.0 * s, kEps);  // sum(C + C^T), floored as _joint_probabilities does
}

// P = max((C + C^T) / sum, eps) off the diagonal, 0 on it, in place: the block of tile pair (ti <= tj) stages both
// tiles, so each unordered pair is read and written by one block; the fp64 sum a + b does not depend on the order.
__global__ __launch_bounds__(kThreads) void tsne_joint_kernel(float* __restrict__ c, int N, const double* __restrict__ total) {
  const int ti = blockIdx.y, tj = blockIdx.x;
  if (tj < ti) return;
  __shared__ float A[32][33];
  __shared__ float B[32][33];
  const int col = threadIdx.x & 31, r0 = threadIdx.x >> 5;
  for (int r = r0; r < 32; r += 8) {
    const int ia = ti * 32 + r, ja = tj * 32 + col, ib = tj * 32 + r, jb = ti * 32 + col;
    A[r][col] = (ia < N && ja < N) ? c[(size_t)ia * N + ja] : 0.0f;
    B[r][col] = (ib < N && jb < N) ? c[(size_t)ib * N + jb] : 0.0f;
  }
  __syncthreads();
  const double sum = total[0];
  for (int r = r0; r < 32; r += 8) {
    const int ia = ti * 32 + r, ja = tj * 32 + col, ib = tj * 32 + r, jb = ti * 32 + col;
    if (ia < N && ja < N) {
      const double v = ((double)A[r][col] + (double)B[col][r]) / sum;
      c[(size_t)ia * N + ja] = ia == ja ? 0.0f : (float)fmax(v, kEps);
    }
    if (ti != tj && ib < N && jb < N) {
      const double v = ((double)A[col][r] + (double)B[r][col]) / sum;
      c[(size_t)ib * N + jb] = (float)fmax(v, kEps);
    }
  }
}

// ------------------------------------------------------------------------------- the descent
constexpr int kPairBlocks = 1536;  // row tiles x column splits aimed at: six blocks per compute unit
constexpr int kPairMaxChunk = 1024;

struct TsnePlan {
  int row_tiles, split, chunk;
  size_t parts_off, z_off, kl_off, gn_off, rowsum_off, total_off, bytes;  // all fp64
};

__host__ TsnePlan tsne_plan(int N) {
  TsnePlan p;
  p.row_tiles = (N + kThreads - 1) / kThreads;
  int split = (kPairBlocks + p.row_tiles - 1) / p.row_tiles;
  const int by_cols = (N + 63) / 64;
  if (split > by_cols) split = by_cols;
  p.chunk = (N + split - 1) / split;
  p.split = (N + p.chunk - 1) / p.chunk;
  size_t off = 0;
  p.parts_off = off; off += (size_t)p.split * 2 * N;
  p.z_off = off; off += (size_t)p.row_tiles * p.split;
  p.kl_off = off; off += (size_t)p.row_tiles * p.split;
  p.gn_off = off; off += (size_t)p.row_tiles;
  p.rowsum_off = off; off += (size_t)N;
  p.total_off = off; off += 2;
  p.bytes = off * sizeof(double);
  return p;
}

// Z pass over the pairs of one (row tile, column split): the block's share of Z = sum_{i != j} n_ij,
// n_ij = 1 / (1 + |y_i - y_j|^2), in fp64.  zpart[row tile * split + s].  Reads the embedding only.
__global__ __launch_bounds__(kThreads) void tsne_z_kernel(const float* __restrict__ y, int N, int chunk,
                                                          double* __restrict__ zpart, const air_tsne_status* __restrict__ st) {
  if (st->stopped) return;
  __shared__ double2 ys[kPairMaxChunk];
  __shared__ double sh[kThreads / 64];
  const int s = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
  const int j0 = s * chunk, j1 = j0 + chunk < N ? j0 + chunk : N;
  for (int j = j0 + threadIdx.x; j < j1; j += kThreads) ys[j - j0] = make_double2((double)y[2 * j], (double)y[2 * j + 1]);
  __syncthreads();
  double z = 0.0;
  if (i < N) {
    const double yx = (double)y[2 * i], yy = (double)y[2 * i + 1];
    for (int j = j0; j < j1; ++j) {
      const double2 yj = ys[j - j0];
      const double dx = yx - yj.x, dy = yy - yj.y;
      const double n = 1.0 / (1.0 + (dx * dx + dy * dy));
      z += j == i ? 0.0 : n;
    }
  }
  z = block_sum_d(z, sh);
  if (threadIdx.x == 0) zpart[blockIdx.x * gridDim.y + s] = z;
}

// Gradient pass over the same blocks, behind the Z pass: per row the sum over the split's columns of
// (e * p_ij - q_ij) * n_ij * (y_i - y_j), q_ij = max(n_ij / Z, eps) - _kl_divergence's terms, floor included - in fp64,
// in column order.  parts[(s * 2 + c) * N + i].  Every block adds the zpart in one fixed order for Z.
__global__ __launch_bounds__(kThreads) void tsne_pair_kernel(const float* __restrict__ P, const float* __restrict__ y, int N,
                                                             int chunk, float ex, const double* __restrict__ zpart, int nz,
                                                             double* __restrict__ parts, const air_tsne_status* __restrict__ st) {
  if (st->stopped) return;
  __shared__ double2 ys[kPairMaxChunk];
  __shared__ double sh[kThreads / 64];
  const double Z = block_sum_array_d(zpart, nz, sh);
  const int s = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
  const int j0 = s * chunk, j1 = j0 + chunk < N ? j0 + chunk : N;
  for (int j = j0 + threadIdx.x; j < j1; j += kThreads) ys[j - j0] = make_double2((double)y[2 * j], (double)y[2 * j + 1]);
  __syncthreads();
  if (i >= N) return;
  double gx = 0.0, gy = 0.0;
  const double yx = (double)y[2 * i], yy = (double)y[2 * i + 1], e = (double)ex;
  const float* __restrict__ p = P + (size_t)j0 * N + i;
  for (int j = j0; j < j1; ++j, p += N) {
    const double2 yj = ys[j - j0];
    const double dx = yx - yj.x, dy = yy - yj.y;  // (j == i: both 0, the term vanishes)
    const double n = 1.0 / (1.0 + (dx * dx + dy * dy));
    const double w = (e * (double)p[0] - fmax(n / Z, kEps)) * n;
    gx = fma(w, dx, gx);
    gy = fma(w, dy, gy);
  }
  double* o = parts + (size_t)s * 2 * N + i;
  o[0] = gx;
  o[(size_t)N] = gy;
}

// KL value of _kl_divergence over the same blocks, all in fp64: sum over ordered pairs of p * log(max(p, eps) / q),
// p = e * p_ij, q = max(n_ij / Z, eps).  Runs behind tsne_pair_kernel of the same embedding (Z from its zpart).
__global__ __launch_bounds__(kThreads) void tsne_kl_kernel(const float* __restrict__ P, const float* __restrict__ y, int N,
                                                           int chunk, float ex, const double* __restrict__ zpart, int nz,
                                                           double* __restrict__ klpart, const air_tsne_status* __restrict__ st) {
  if (st->stopped) return;
  __shared__ double2 ys[kPairMaxChunk];
  __shared__ double sh[kThreads / 64];
  const double Z = block_sum_array_d(zpart, nz, sh);
  const int s = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
  const int j0 = s * chunk, j1 = j0 + chunk < N ? j0 + chunk : N;
  for (int j = j0 + threadIdx.x; j < j1; j += kThreads) ys[j - j0] = make_double2((double)y[2 * j], (double)y[2 * j + 1]);
  __syncthreads();
  double kl = 0.0;
  if (i < N) {
    const double yx = (double)y[2 * i], yy = (double)y[2 * i + 1];
    const float* __restrict__ p = P + (size_t)j0 * N + i;
    for (int j = j0; j < j1; ++j, p += N) {
      if (j == i) continue;
      const double2 yj = ys[j - j0];
      const double dx = yx - yj.x, dy = yy - yj.y;
      const double n = 1.0 / (1.0 + (dx * dx + dy * dy));
      const double q = fmax(n / Z, kEps);
      const double pe = (double)ex * (double)p[0];
      kl = fma(pe, log(fmax(pe, kEps) / q), kl);
    }
  }
  kl = block_sum_d(kl, sh);
  if (threadIdx.x == 0) klpart[blockIdx.x * gridDim.y + s] = kl;
}

// gradient of row i: 4 * the sum of its split partials, in split order
__device__ __forceinline__ void tsne_row_grad(const double* __restrict__ parts, int N, int split, int i, double& gx, double& gy) {
  double ax = 0.0, ay = 0.0;
  for (int s = 0; s < split; ++s) {
    const double* o = parts + (size_t)s * 2 * N + i;
    ax += o[0];
    ay += o[(size_t)N];
  }
  gx = 4.0 * ax;
  gy = 4.0 * ay;
}

__global__ __launch_bounds__(kThreads) void tsne_grad_kernel(const double* __restrict__ parts, int N, int split,
                                                             float* __restrict__ grad) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= N) return;
  double gx, gy;
  tsne_row_grad(parts, N, split, i, gx, gy);
  grad[2 * i] = (float)gx;
  grad[2 * i + 1] = (float)gy;
}

// _gradient_descent's update: inc = update * grad < 0; gains += 0.2 there, *= 0.8 elsewhere, floored at 0.01;
// grad *= gains; update = momentum * update - lr * grad; y += update - the state (y, update, gains) is fp32, each new
// value is formed in fp64 from the fp64 gradient and rounded once.  gnpart[block] = sum of (gains * grad)^2: the norm
// _gradient_descent tests is taken after grad *= gains.
__device__ __forceinline__ double tsne_update_one(double g, double momentum, double lr, float& u, float& gain, float& yv) {
  const double ga = fmax(((double)u * g < 0.0) ? (double)gain + 0.2 : (double)gain * 0.8, 0.01);
  gain = (float)ga;
  const double gg = g * ga;
  u = (float)(momentum * (double)u - lr * gg);
  yv = (float)((double)yv + (double)u);
  return gg * gg;
}

__global__ __launch_bounds__(kThreads) void tsne_update_kernel(const double* __restrict__ parts, int N, int split,
                                                               float momentum, float lr,
                                                               float* __restrict__ y, float* __restrict__ update,
                                                               float* __restrict__ gains, double* __restrict__ gnpart,
                                                               const air_tsne_status* __restrict__ st) {
  if (st->stopped) return;
  __shared__ double sh[kThreads / 64];
  const int i = blockIdx.x * kThreads + threadIdx.x;
  double gn = 0.0;
  if (i < N) {
    double gx, gy;
    tsne_row_grad(parts, N, split, i, gx, gy);
    float u0 = update[2 * i], u1 = update[2 * i + 1], g0 = gains[2 * i], g1 = gains[2 * i + 1];
    float y0 = y[2 * i], y1 = y[2 * i + 1];
    gn = tsne_update_one(gx, momentum, lr, u0, g0, y0);
    gn += tsne_update_one(gy, momentum, lr, u1, g1, y1);
    update[2 * i] = u0; update[2 * i + 1] = u1;
    gains[2 * i] = g0; gains[2 * i + 1] = g1;
    y[2 * i] = y0; y[2 * i + 1] = y1;
  }
  gn = block_sum_d(gn, sh);
  if (threadIdx.x == 0) gnpart[blockIdx.x] = gn;
}

// One block behind the update of iteration `iter`: records the KL (NaN when it was not computed) and the norm of
// gains * grad, and with apply_rules evaluates _gradient_descent's stop rules on the status record.
__global__ __launch_bounds__(kThreads) void tsne_check_kernel(const double* __restrict__ klpart, int nkl, int have_kl,
                                                              const double* __restrict__ gnpart, int ngn, int iter,
                                                              int apply_rules, int n_iter_without_progress,
                                                              double min_grad_norm, air_tsne_status* __restrict__ st) {
  if (st->stopped) return;
  __shared__ double sh[kThreads / 64];
  const double kl = have_kl ? block_sum_array_d(klpart, nkl, sh) : (double)NAN;
  const double gn = sqrt(block_sum_array_d(gnpart, ngn, sh));
  if (threadIdx.x != 0) return;
  st->kl = kl;
  st->grad_norm = gn;
  st->n_iter = iter;
  if (!apply_rules) return;
  if (kl < st->best_error) {
    st->best_error = kl;
    st->best_iter = iter;
  } else if (iter - st->best_iter > n_iter_without_progress) {
    st->stopped = 1;
    st->reason = 1;
    return;
  }
  if (gn <= min_grad_norm) {
    st->stopped = 1;
    st->reason = 2;
  }
}

// the start of one _gradient_descent call at iteration `iter`: update = 0, gains = 1, the best error forgotten;
// first: the record itself is initialised
__global__ __launch_bounds__(kThreads) void tsne_reset_kernel(float* __restrict__ update, float* __restrict__ gains, int n2,
                                                              int iter, int first, air_tsne_status* __restrict__ st) {
  if (!first && st->stopped) return;
  const int e = blockIdx.x * kThreads + threadIdx.x;
  if (e < n2) {
    update[e] = 0.0f;
    gains[e] = 1.0f;
  }
  if (e == 0) {
    if (first) {
      st->stopped = 0;
      st->reason = 0;
      st->n_iter = 0;
      st->kl = (double)NAN;
      st->grad_norm = (double)NAN;
      st->pad[0] = st->pad[1] = st->pad[2] = 0.0;
    }
    st->best_error = DBL_MAX;
    st->best_iter = iter;
  }
}

bool vis_n_ok(int N) { return N >= 2 && N <= kVisMaxN; }

}  // namespace

extern "C" {

int air_vis_max_n(void) { return kVisMaxN; }
int air_vis_max_d(void) { return kVisMaxD; }
int air_pca_max_components(void) { return kPcaMaxK; }

size_t air_pca_ws_bytes(int N, int D) {
  if (!vis_n_ok(N) || D < 1 || D > kVisMaxD) return 0;
  return pca_plan(N, D).bytes;
}

int air_pca_gram(const float* x, int N, int D, float* mean, double* gram, void* ws, size_t ws_bytes, air_stream_t stream) {
  if (D < 1) return AIR_EINVAL;
  if (!vis_n_ok(N) || D > kVisMaxD) return AIR_EUNSUPPORTED;
  if (!x || !mean || !gram || !ws || ((uintptr_t)ws & 15)) return AIR_EINVAL;
  const PcaPlan p = pca_plan(N, D);
  if (ws_bytes < p.bytes) return AIR_EWORKSPACE;
  hipStream_t st = air_stream(stream);
  double* colsum = reinterpret_cast<double*>(static_cast<char*>(ws) + p.colsum_off);
  double* part = reinterpret_cast<double*>(static_cast<char*>(ws) + p.gram_off);
  const int dblocks = (D + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(pca_colsum_kernel, dim3(dblocks, p.chunks), dim3(kThreads), 0, st, x, N, D, p.rows_per_chunk, colsum);
  hipLaunchKernelGGL(pca_mean_kernel, dim3(dblocks), dim3(kThreads), 0, st, colsum, N, D, p.chunks, mean);
  hipLaunchKernelGGL(pca_gram_kernel, dim3(p.tiles, p.tiles, p.split), dim3(kThreads), 0, st, x, mean, N, D, p.rows_per_split,
                     part);
  hipLaunchKernelGGL(pca_gram_reduce_kernel, dim3((unsigned)(((size_t)D * D + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                     part, D, p.split, gram);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

int air_pca_project(const float* x, int N, int D, const float* mean, const float* comps, int K, float* out,
                    air_stream_t stream) {
  if (D < 1 || K < 1) return AIR_EINVAL;
  if (!vis_n_ok(N) || D > kVisMaxD || K > kPcaMaxK) return AIR_EUNSUPPORTED;
  if (!x || !mean || !comps || !out) return AIR_EINVAL;
  hipLaunchKernelGGL(pca_project_kernel, dim3((N + 3) / 4), dim3(kThreads), 0, air_stream(stream), x, mean, comps, N, D, K, out);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

int air_pairwise_sqdist(const float* x, int N, int D, float* out, air_stream_t stream) {
  if (D < 1) return AIR_EINVAL;
  if (!vis_n_ok(N) || D > kVisMaxD) return AIR_EUNSUPPORTED;
  if (!x || !out) return AIR_EINVAL;
  const int tiles = (N + kDistTile - 1) / kDistTile;
  const dim3 grid(tiles, tiles), block(kThreads);
  if (D % 4 == 0 && ((uintptr_t)x & 15) == 0)
    hipLaunchKernelGGL(sqdist_kernel<true>, grid, block, 0, air_stream(stream), x, N, D, out);
  else
    hipLaunchKernelGGL(sqdist_kernel<false>, grid, block, 0, air_stream(stream), x, N, D, out);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

int air_tsne_affinities(const float* dist, int N, float perplexity, float* cond, float* beta, air_stream_t stream) {
  if (!(perplexity > 0.0f)) return AIR_EINVAL;
  if (!vis_n_ok(N)) return AIR_EUNSUPPORTED;
  if (!dist || !cond || !beta || dist == cond) return AIR_EINVAL;
  hipLaunchKernelGGL(tsne_affinity_kernel, dim3(N), dim3(kThreads), 0, air_stream(stream), dist, N, std::log((double)perplexity),
                     cond, beta);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

size_t air_tsne_ws_bytes(int N) {
  if (!vis_n_ok(N)) return 0;
  return tsne_plan(N).bytes;
}

#define AIR_TSNE_ARGS_OK()                                                  \
  if (!vis_n_ok(N)) return AIR_EUNSUPPORTED;                                \
  const TsnePlan p = tsne_plan(N);                                          \
  if (p.chunk > kPairMaxChunk) return AIR_EUNSUPPORTED;                     \
  if (!ws || ((uintptr_t)ws & 15)) return AIR_EINVAL;                       \
  if (ws_bytes < p.bytes) return AIR_EWORKSPACE;                            \
  double* w = static_cast<double*>(ws);                                     \
  hipStream_t hs = air_stream(stream);                                      \
  (void)w; (void)hs

int air_tsne_joint(float* P, int N, void* ws, size_t ws_bytes, air_stream_t stream) {
  AIR_TSNE_ARGS_OK();
  if (!P) return AIR_EINVAL;
  hipLaunchKernelGGL(tsne_rowsum_kernel, dim3(N), dim3(kThreads), 0, hs, P, N, w + p.rowsum_off);
  hipLaunchKernelGGL(tsne_total_kernel, dim3(1), dim3(kThreads), 0, hs, w + p.rowsum_off, N, w + p.total_off);
  const int tiles = (N + 31) / 32;
  hipLaunchKernelGGL(tsne_joint_kernel, dim3(tiles, tiles), dim3(kThreads), 0, hs, P, N, w + p.total_off);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

int air_tsne_begin(float* update, float* gains, int N, int iter, int first, air_tsne_status* status, air_stream_t stream) {
  if (iter < 0) return AIR_EINVAL;
  if (!vis_n_ok(N)) return AIR_EUNSUPPORTED;
  if (!update || !gains || !status) return AIR_EINVAL;
  hipLaunchKernelGGL(tsne_reset_kernel, dim3((2 * N + kThreads - 1) / kThreads), dim3(kThreads), 0, air_stream(stream), update,
                     gains, 2 * N, iter, first ? 1 : 0, status);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

int air_tsne_pairs(const float* P, const float* y, int N, float exaggeration, int want_kl, const air_tsne_status* status,
                   void* ws, size_t ws_bytes, air_stream_t stream) {
  AIR_TSNE_ARGS_OK();
  if (!P || !y || !status) return AIR_EINVAL;
  const dim3 grid(p.row_tiles, p.split), block(kThreads);
  hipLaunchKernelGGL(tsne_z_kernel, grid, block, 0, hs, y, N, p.chunk, w + p.z_off, status);
  hipLaunchKernelGGL(tsne_pair_kernel, grid, block, 0, hs, P, y, N, p.chunk, exaggeration, w + p.z_off, p.row_tiles * p.split,
                     w + p.parts_off, status);
  if (want_kl)
    hipLaunchKernelGGL(tsne_kl_kernel, grid, block, 0, hs, P, y, N, p.chunk, exaggeration, w + p.z_off, p.row_tiles * p.split,
                       w + p.kl_off, status);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

int air_tsne_gradient(int N, float* grad, void* ws, size_t ws_bytes, air_stream_t stream) {
  AIR_TSNE_ARGS_OK();
  if (!grad) return AIR_EINVAL;
  hipLaunchKernelGGL(tsne_grad_kernel, dim3(p.row_tiles), dim3(kThreads), 0, hs, w + p.parts_off, N, p.split, grad);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

int air_tsne_update(float* y, float* update, float* gains, int N, float momentum, float learning_rate,
                    const air_tsne_status* status, void* ws, size_t ws_bytes, air_stream_t stream) {
  AIR_TSNE_ARGS_OK();
  if (!y || !update || !gains || !status) return AIR_EINVAL;
  hipLaunchKernelGGL(tsne_update_kernel, dim3(p.row_tiles), dim3(kThreads), 0, hs, w + p.parts_off, N, p.split, momentum,
                     learning_rate, y, update, gains, w + p.gn_off, status);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

int air_tsne_check(int N, int iter, int have_kl, int apply_rules, int n_iter_without_progress, double min_grad_norm,
                   air_tsne_status* status, void* ws, size_t ws_bytes, air_stream_t stream) {
  AIR_TSNE_ARGS_OK();
  if (!status || iter < 0) return AIR_EINVAL;
  hipLaunchKernelGGL(tsne_check_kernel, dim3(1), dim3(kThreads), 0, hs, w + p.kl_off, p.row_tiles * p.split, have_kl ? 1 : 0,
                     w + p.gn_off, p.row_tiles, iter, apply_rules ? 1 : 0, n_iter_without_progress, min_grad_norm, status);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

int air_tsne_run(const float* P, float* y, float* update, float* gains, int N, const air_tsne_schedule* s,
                 air_tsne_status* status, void* ws, size_t ws_bytes, air_stream_t stream) {
  if (!s) return AIR_EINVAL;
  if (s->max_iter < 1 || s->exploration_iter < 0 || s->n_iter_check < 1 || s->n_iter_without_progress < 0 ||
      !(s->learning_rate > 0.0f) || !(s->early_exaggeration > 0.0f))
    return AIR_EINVAL;
  int rc = air_tsne_begin(update, gains, N, 0, 1, status, stream);
  for (int i = 0; rc == AIR_OK && i < s->max_iter; ++i) {
    const bool second = i >= s->exploration_iter;
    if (i > 0 && i == s->exploration_iter) rc = air_tsne_begin(update, gains, N, i, 0, status, stream);
    const bool check = second && (i + 1) % s->n_iter_check == 0;
    const bool want_kl = check || i == s->max_iter - 1;
    if (rc == AIR_OK)
      rc = air_tsne_pairs(P, y, N, second ? 1.0f : s->early_exaggeration, want_kl, status, ws, ws_bytes, stream);
    if (rc == AIR_OK)
      rc = air_tsne_update(y, update, gains, N, second ? 0.8f : 0.5f, s->learning_rate, status, ws, ws_bytes, stream);
    if (rc == AIR_OK && want_kl)
      rc = air_tsne_check(N, i, 1, check, s->n_iter_without_progress, s->min_grad_norm, status, ws, ws_bytes, stream);
  }
  return rc;
}

}  // extern "C"
