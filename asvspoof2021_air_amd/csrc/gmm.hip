// Diagonal-covariance GMM back-end: fp64 EM statistics and log-likelihood scoring (include/air_hip.h, "GMM back-end",
// is the specification; tests/gmm_oracle.py states it in numpy).
//
// Everything that is a matrix product runs on v_mfma_f64_16x16x4_f64.  Its maps (cdna_hip_programming.md, "Fragment
// layout"; held by the exact-integer tests of tests/test_gmm_gpu.py): lane l gives A[row l & 15][k l >> 4] and
// B[k l >> 4][col l & 15], one double each, and receives D[row (l >> 4) + 4 i][col l & 15] in result i = 0 .. 3 - NOT
// the f32 forms' row (l >> 4) * 4 + i.
//
//   logits   (frames x 2 Dp) . (2 Dp x components): A = [x, x^2] widened from an fp32 LDS tile (x^2 is exact in fp64),
//            B = the packed model [mu p; -0.5 p], read coalesced from memory, 64 doubles per k-step.
//   sums     (components x frames) . (frames x 2 Dp): result i of the logit tile holds, for the lane's component
//            l & 15, the frames (l >> 4) + 4 i - exactly the A operand [component][k = l >> 4] of a product over the
//            frames {4 i' + (l >> 4)}.  So r = exp(logit - lse) goes from the accumulator into the next MFMA with no
//            lane movement and no LDS; B = [x, x^2][frame (l >> 4) + 4 i][feature l & 15].
//
// Pass A (gmm_lse_kernel), one workgroup per tile of 64 frames: the component tiles are dealt over the four waves,
//   every lane keeps a running (max, sum) per frame it sees, merged once per workgroup through LDS (maximum first, so
//   the merge costs one exp per running pair).  Writes lse per frame and one (sum lse, count) pair per tile.
// Pass B (gmm_stats_kernel), grid (frame chunks x 64-component chunks): a wave holds its 16 components' operand
//   (Dp / 2 doubles per lane) and their 16 x 2 Dp sums (Dp / 4 doubles per lane) in registers over the whole chunk,
//   recomputes the logits, and writes one partial per chunk.  The responsibilities exist only in registers.
// Pass C (gmm_merge_kernel, gmm_ll_merge_kernel): adds the partials in chunk / tile order into stats.  No atomics
//   anywhere: equal calls give equal bits.
#include "air_common.h"

#include <cfloat>
#include <cmath>

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int kFT = 64;         // frames per LDS tile (4 MFMA row tiles)
constexpr int kXS = kFT + 16;   // LDS row stride of the [feature][frame] tile: the logit product's reads fall on 64 banks
constexpr int kMaxK = 1024, kMaxD = 128;
constexpr int kThreads = 256;
constexpr int kStatWgs = 512;   // workgroups pass B aims at: two rounds of one 4-wave workgroup per CU

inline int gmm_dp(int D) { return D <= 8 ? 8 : D <= 32 ? 32 : D <= 64 ? 64 : 128; }
inline bool gmm_shape_ok(int K, int D) { return K >= 1 && K <= kMaxK && D >= 1 && D <= kMaxD; }
inline int64_t gmm_tiles(int64_t n) { return (n + kFT - 1) / kFT; }
inline int64_t gmm_chunks(int64_t ntiles, int K) {
  const int kt4 = ((K + 15) / 16 + 3) / 4;
  const int64_t want = kStatWgs / kt4 > 0 ? kStatWgs / kt4 : 1;
  return ntiles < want ? ntiles : want;
}
inline size_t gmm_partial_doubles(int K, int D) {  // one chunk's partial: (Kp, 2 Dp) sums, then Kp counts
  const size_t Kp = (size_t)((K + 15) / 16) * 16;
  return Kp * 2 * gmm_dp(D) + Kp;
}

struct GmmWs {
  double* lse;
  double* ll_part;
  long long* cnt_part;
  double* part;
  size_t bytes;
};
inline GmmWs gmm_ws_layout(void* ws, int64_t n, int K, int D) {
  GmmWs w;
  const int64_t nt = gmm_tiles(n);
  char* p = (char*)ws;
  w.lse = (double*)p;
  p += (size_t)n * 8;
  w.ll_part = (double*)p;
  p += (size_t)nt * 8;
  w.cnt_part = (long long*)p;
  p += (size_t)nt * 8;
  w.part = (double*)p;
  p += (size_t)gmm_chunks(nt, K) * gmm_partial_doubles(K, D) * 8;
  w.bytes = (size_t)(p - (char*)ws);
  return w;
}

// ------------------------------------------------------------------------------------------------------ prepare
// One workgroup per (padded) component.
__global__ __launch_bounds__(kThreads) void gmm_prepare_kernel(const double* __restrict__ w, const double* __restrict__ mu,
                                                               const double* __restrict__ var, int K, int D, int Dp,
                                                               double* __restrict__ params) {
  const int k = blockIdx.x, kt = k >> 4, col = k & 15;
  const int Kp = gridDim.x;
  double* P = params + (size_t)kt * (2 * Dp * 16);
  for (int j = threadIdx.x; j < 2 * Dp; j += kThreads) {
    const int d = j < Dp ? j : j - Dp;
    double v = 0.0;
    if (k < K && d < D) {
      const double p = 1.0 / var[(size_t)k * D + d];
      v = j < Dp ? mu[(size_t)k * D + d] * p : -0.5 * p;
    }
    P[j * 16 + col] = v;
  }
  if (threadIdx.x == 0) {
    double c = -INFINITY;
    if (k < K) {
      double sm = 0.0, sl = 0.0;
      for (int d = 0; d < D; ++d) {
        const double m = mu[(size_t)k * D + d], v = var[(size_t)k * D + d];
        sm += m * m * (1.0 / v);
        sl += log(v);
      }
      c = log(w[k]) - 0.5 * ((double)D * 1.8378770664093453 /* log(2 pi) */ + sm + sl);
    }
    params[(size_t)Kp * 2 * Dp + k] = c;
  }
}

// ------------------------------------------------------------------------------------------------- shared tile code
struct Frames {
  const float* x;
  const int* n_frames;
  int layout, B, Tcap, D, Dp;
  int64_t n;  // B * Tcap
};

// Frame g of the flattened (B, Tcap) index: valid (inside its row's count) and the element offset of its feature 0.
__device__ __forceinline__ void gmm_frame(const Frames& f, int64_t g, int& valid, int64_t& base) {
  valid = 0;
  base = 0;
  if (g >= f.n) return;
  const int b = (int)(g / f.Tcap), t = (int)(g - (int64_t)b * f.Tcap);
  int nf = f.Tcap;
  if (f.n_frames) {
    nf = f.n_frames[b];
    nf = nf < 0 ? 0 : nf > f.Tcap ? f.Tcap : nf;
  }
  valid = t < nf;
  base = f.layout == 0 ? g * f.D : (int64_t)b * f.D * f.Tcap + t;
}

// xs[d][frame] <- the tile's frames, zeros for padding features and for frames that do not count (never loaded).
__device__ __forceinline__ void gmm_load_tile(const Frames& f, const int* valid_s, const int64_t* base_s, float* xs) {
  const int total = kFT * f.Dp;
  if (f.layout == 0) {
    for (int idx = threadIdx.x; idx < total; idx += kThreads) {
      const int fr = idx / f.Dp, d = idx - fr * f.Dp;
      xs[d * kXS + fr] = (d < f.D && valid_s[fr]) ? f.x[base_s[fr] + d] : 0.0f;
    }
  } else {
    for (int idx = threadIdx.x; idx < total; idx += kThreads) {
      const int d = idx / kFT, fr = idx - d * kFT;
      xs[d * kXS + fr] = (d < f.D && valid_s[fr]) ? f.x[base_s[fr] + (int64_t)d * f.Tcap] : 0.0f;
    }
  }
}

// -------------------------------------------------------------------------------------------------------- pass A
__global__ __launch_bounds__(kThreads) void gmm_lse_kernel(Frames f, const double* __restrict__ params, int KT,
                                                           double* __restrict__ lse_out, double* __restrict__ ll_part,
                                                           long long* __restrict__ cnt_part) {
  __shared__ float xs[kMaxD * kXS];
  __shared__ double red[4][kFT];
  __shared__ double mxs[kFT];
  __shared__ int64_t base_s[kFT];
  __shared__ int valid_s[kFT];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 15, q = lane >> 4;
  const int64_t g0 = (int64_t)blockIdx.x * kFT;
  int v = 0;
  if (tid < kFT) {
    int64_t base;
    gmm_frame(f, g0 + tid, v, base);
    valid_s[tid] = v;
    base_s[tid] = base;
  }
  const int any = __syncthreads_or(v);
  if (!any) {  // nothing counts in this tile (a row routed to the other model, padding): no arithmetic
    if (tid < kFT && g0 + tid < f.n) lse_out[g0 + tid] = 0.0;
    if (tid == 0) {
      ll_part[blockIdx.x] = 0.0;
      cnt_part[blockIdx.x] = 0;
    }
    return;
  }
  gmm_load_tile(f, valid_s, base_s, xs);
  __syncthreads();

  const int Dp = f.Dp, nsteps = Dp >> 1;
  const double* cvec = params + (size_t)KT * 16 * 2 * Dp;
  double rm[4][4], rs[4][4];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      rm[m][i] = -DBL_MAX;
      rs[m][i] = 0.0;
    }
  for (int kt = wave; kt < KT; kt += 4) {
    const double* P = params + (size_t)kt * (2 * Dp * 16) + q * 16 + col;
    d4 acc[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) acc[m] = (d4){0.0, 0.0, 0.0, 0.0};
    for (int s = 0; s < nsteps; ++s) {
      const double bv = P[s * 64];
      const int j = 4 * s + q;
      const bool sq = j >= Dp;
      const float* xr = xs + (sq ? j - Dp : j) * kXS + col;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const double xv = (double)xr[16 * m];
        acc[m] = __builtin_amdgcn_mfma_f64_16x16x4f64(sq ? xv * xv : xv, bv, acc[m], 0, 0, 0);
      }
    }
    const double ck = cvec[kt * 16 + col];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const double lp = acc[m][i] + ck;
        const double d = lp - rm[m][i];
        const double e = exp(-fabs(d));
        rs[m][i] = d > 0.0 ? fma(rs[m][i], e, 1.0) : rs[m][i] + e;
        rm[m][i] = fmax(rm[m][i], lp);
      }
  }
  // the frame's maximum over the 16 component lanes, then over the waves
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      double mx = rm[m][i];
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
      if (col == 0) red[wave][16 * m + q + 4 * i] = mx;
    }
  __syncthreads();
  double t[4][4];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int fr = 16 * m + q + 4 * i;
      const double M = fmax(fmax(red[0][fr], red[1][fr]), fmax(red[2][fr], red[3][fr]));
      double ts = rs[m][i] * exp(rm[m][i] - M);
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) ts += __shfl_xor(ts, o, 64);
      t[m][i] = ts;
      if (wave == 0 && col == 0) mxs[fr] = M;
    }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (col == 0) red[wave][16 * m + q + 4 * i] = t[m][i];
  __syncthreads();
  if (wave == 0) {
    const int fr = lane;
    const double S = ((red[0][fr] + red[1][fr]) + red[2][fr]) + red[3][fr];
    const double l = valid_s[fr] ? mxs[fr] + log(S) : 0.0;
    if (g0 + fr < f.n) lse_out[g0 + fr] = l;
    const double ll = air_wave_sum_d(l);
    const unsigned long long bal = __ballot(valid_s[fr] != 0);
    if (lane == 0) {
      ll_part[blockIdx.x] = ll;
      cnt_part[blockIdx.x] = (long long)__popcll(bal);
    }
  }
}

// -------------------------------------------------------------------------------------------------------- pass B
// NJT = Dp / 8: the wave's 2 Dp features are NJT column tiles of 16, the logit product has 4 NJT k-steps.
template <int NJT>
__global__ __launch_bounds__(kThreads) void gmm_stats_kernel(Frames f, const double* __restrict__ params, int KT,
                                                             const double* __restrict__ lse, int64_t ntiles,
                                                             double* __restrict__ part, size_t part_doubles) {
  constexpr int Dp = 8 * NJT;
  __shared__ float xs[Dp * kXS];
  __shared__ double lse_s[kFT];
  __shared__ int64_t base_s[kFT];
  __shared__ int valid_s[kFT];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 15, q = lane >> 4;
  const int kt = blockIdx.y * 4 + wave;
  const bool active = kt < KT;
  const int nchunks = gridDim.x;
  const int64_t t0 = ntiles * blockIdx.x / nchunks, t1 = ntiles * (blockIdx.x + 1) / nchunks;

  double Pr[4 * NJT];
  double ck = 0.0;
  if (active) {
    const double* P = params + (size_t)kt * (2 * Dp * 16) + q * 16 + col;
#pragma unroll
    for (int s = 0; s < 4 * NJT; ++s) Pr[s] = P[s * 64];
    ck = params[(size_t)KT * 16 * 2 * Dp + kt * 16 + col];
  } else {
#pragma unroll
    for (int s = 0; s < 4 * NJT; ++s) Pr[s] = 0.0;
  }
  d4 S[NJT];
#pragma unroll
  for (int jt = 0; jt < NJT; ++jt) S[jt] = (d4){0.0, 0.0, 0.0, 0.0};
  double s0 = 0.0;

  for (int64_t tile = t0; tile < t1; ++tile) {
    const int64_t g0 = tile * kFT;
    __syncthreads();  // the previous tile's readers are done
    int v = 0;
    if (tid < kFT) {
      int64_t base;
      gmm_frame(f, g0 + tid, v, base);
      valid_s[tid] = v;
      base_s[tid] = base;
      lse_s[tid] = v ? lse[g0 + tid] : INFINITY;  // exp(lp - inf) = 0: the frame carries no responsibility
    }
    const int any = __syncthreads_or(v);
    if (!any) continue;
    gmm_load_tile(f, valid_s, base_s, xs);
    __syncthreads();
    if (!active) continue;
#pragma unroll 1
    for (int m = 0; m < 4; ++m) {
      d4 acc = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s = 0; s < 4 * NJT; ++s) {  // the order and operands of pass A: the same bits
        const int j = 4 * s + q;
        const bool sq = j >= Dp;
        const double xv = (double)xs[(sq ? j - Dp : j) * kXS + 16 * m + col];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(sq ? xv * xv : xv, Pr[s], acc, 0, 0, 0);
      }
      double r[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        r[i] = exp((acc[i] + ck) - lse_s[16 * m + q + 4 * i]);
        s0 += r[i];
      }
#pragma unroll
      for (int jt = 0; jt < NJT; ++jt) {
        const int j = 16 * jt + col;
        const bool sq = j >= Dp;
        const float* xr = xs + (sq ? j - Dp : j) * kXS + 16 * m + q;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const double xv = (double)xr[4 * i];
          S[jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(r[i], sq ? xv * xv : xv, S[jt], 0, 0, 0);
        }
      }
    }
  }
  if (!active) return;
  double* out = part + (size_t)blockIdx.x * part_doubles;
#pragma unroll
  for (int jt = 0; jt < NJT; ++jt)
#pragma unroll
    for (int i = 0; i < 4; ++i) out[(size_t)(kt * 16 + q + 4 * i) * (2 * Dp) + 16 * jt + col] = S[jt][i];
  s0 += __shfl_xor(s0, 16, 64);
  s0 += __shfl_xor(s0, 32, 64);
  if (q == 0) out[(size_t)KT * 16 * 2 * Dp + kt * 16 + col] = s0;
}

// -------------------------------------------------------------------------------------------------------- pass C
// One thread per entry of S0 | S1 | S2: the chunks' partials in chunk order, then onto stats.
__global__ __launch_bounds__(kThreads) void gmm_merge_kernel(const double* __restrict__ part, size_t part_doubles,
                                                             int nchunks, int K, int D, int Dp, int Kp,
                                                             double* __restrict__ stats) {
  const int idx = blockIdx.x * kThreads + threadIdx.x;
  const int total = K + 2 * K * D;
  if (idx >= total) return;
  size_t src;
  if (idx < K) {
    src = (size_t)Kp * 2 * Dp + idx;
  } else {
    const int e = idx - K, which = e / (K * D), kd = e - which * K * D, k = kd / D, d = kd - k * D;
    src = (size_t)k * 2 * Dp + which * Dp + d;
  }
  double s = 0.0;
  for (int c = 0; c < nchunks; ++c) s += part[(size_t)c * part_doubles + src];
  stats[idx] += s;
}

// LL and Nf: one workgroup; thread t adds the tiles t, t + 256, .. in order, then a fixed tree.
__global__ __launch_bounds__(kThreads) void gmm_ll_merge_kernel(const double* __restrict__ ll_part,
                                                                const long long* __restrict__ cnt_part, int64_t ntiles,
                                                                double* __restrict__ ll, long long* __restrict__ nf) {
  __shared__ double sl[kThreads];
  __shared__ long long sc[kThreads];
  double a = 0.0;
  long long c = 0;
  for (int64_t t = threadIdx.x; t < ntiles; t += kThreads) {
    a += ll_part[t];
    c += cnt_part[t];
  }
  sl[threadIdx.x] = a;
  sc[threadIdx.x] = c;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      sl[threadIdx.x] += sl[threadIdx.x + o];
      sc[threadIdx.x] += sc[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    *ll += sl[0];
    *nf += sc[0];
  }
}

// Row b's mean of lse over its frames (NaN without frames): thread-strided sums in order, then a fixed tree.
__global__ __launch_bounds__(kThreads) void gmm_row_mean_kernel(const double* __restrict__ lse, int Tcap,
                                                                const int* __restrict__ n_frames,
                                                                double* __restrict__ row_ll) {
  __shared__ double sl[kThreads];
  const int b = blockIdx.x;
  int nf = Tcap;
  if (n_frames) {
    nf = n_frames[b];
    nf = nf < 0 ? 0 : nf > Tcap ? Tcap : nf;
  }
  double a = 0.0;
  for (int t = threadIdx.x; t < nf; t += kThreads) a += lse[(int64_t)b * Tcap + t];
  sl[threadIdx.x] = a;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sl[threadIdx.x] += sl[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) row_ll[b] = sl[0] / (double)nf;
}

// -------------------------------------------------------------------------------------------------------- M-step
// One workgroup per component; each recomputes sum_k nk (K <= 1024 reads) in the same fixed order.
__global__ __launch_bounds__(kThreads) void gmm_mstep_kernel(const double* __restrict__ stats, int K, int D,
                                                             double reg_covar, double* __restrict__ w,
                                                             double* __restrict__ mu, double* __restrict__ var,
                                                             double* __restrict__ lower_bound) {
  __shared__ double sl[kThreads];
  const double tiny = 10.0 * 2.220446049250313e-16;  // 10 * np.finfo(float64).eps
  double a = 0.0;
  for (int k = threadIdx.x; k < K; k += kThreads) a += stats[k] + tiny;
  sl[threadIdx.x] = a;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sl[threadIdx.x] += sl[threadIdx.x + o];
    __syncthreads();
  }
  const double total = sl[0];
  const int k = blockIdx.x;
  const double nk = stats[k] + tiny;
  const double* S1 = stats + K + (size_t)k * D;
  const double* S2 = stats + K + (size_t)K * D + (size_t)k * D;
  for (int d = threadIdx.x; d < D; d += kThreads) {
    const double m = S1[d] / nk;
    mu[(size_t)k * D + d] = m;
    var[(size_t)k * D + d] = (S2[d] / nk - m * m) + reg_covar;
  }
  if (threadIdx.x == 0) {
    w[k] = nk / total;
    if (k == 0) {
      const size_t tail = (size_t)K + 2 * (size_t)K * D;
      const long long nf = *reinterpret_cast<const long long*>(stats + tail + 1);
      *lower_bound = stats[tail] / (double)nf;
    }
  }
}

// Measurement instrumentation: the rate a bare loop of v_mfma_f64_16x16x4_f64 reaches - four independent accumulators
// per wave, four waves per workgroup, no memory traffic inside the loop.  The fp64 matrix peak is in neither guide;
// tools/bench_gmm.py measures it with this beside the kernels it judges.
__global__ __launch_bounds__(kThreads) void gmm_mfma_probe_kernel(int iters, double* __restrict__ out) {
  const double a = 1.0 + 1e-9 * threadIdx.x, b = 1.0 - 1e-9 * threadIdx.x;
  d4 acc[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) acc[m] = (d4){0.0, 0.0, 0.0, 0.0};
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int m = 0; m < 4; ++m) acc[m] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[m], 0, 0, 0);
  }
  double s = 0.0;
#pragma unroll
  for (int m = 0; m < 4; ++m) s += acc[m][0] + acc[m][1] + acc[m][2] + acc[m][3];
  out[(size_t)blockIdx.x * kThreads + threadIdx.x] = s;
}

int gmm_check(const float* x, int layout, int B, int Tcap, const double* params, int K, int D) {
  if (!gmm_shape_ok(K, D)) return AIR_EUNSUPPORTED;
  if ((layout != 0 && layout != 1) || B < 1 || Tcap < 1) return AIR_EINVAL;
  if ((int64_t)B * Tcap >= ((int64_t)1 << 31)) return AIR_EUNSUPPORTED;
  if (!x || !params) return AIR_EINVAL;
  return AIR_OK;
}

int gmm_launch_lse(const Frames& f, const double* params, int K, double* lse_out, double* ll_part, long long* cnt_part,
                   hipStream_t st) {
  const int KT = (K + 15) / 16;
  hipLaunchKernelGGL(gmm_lse_kernel, dim3((unsigned)gmm_tiles(f.n)), dim3(kThreads), 0, st, f, params, KT, lse_out, ll_part,
                     cnt_part);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

}  // namespace

extern "C" {

int air_gmm_frame_tile(void) { return kFT; }

size_t air_gmm_params_doubles(int K, int D) {
  if (!gmm_shape_ok(K, D)) return 0;
  return gmm_partial_doubles(K, D);  // (Kp, 2 Dp) operand + Kp constants: the same count
}

size_t air_gmm_stats_doubles(int K, int D) {
  if (!gmm_shape_ok(K, D)) return 0;
  return (size_t)K + 2 * (size_t)K * D + 2;
}

size_t air_gmm_ws_bytes(int64_t n_frames_cap, int K, int D) {
  if (!gmm_shape_ok(K, D) || n_frames_cap < 1 || n_frames_cap >= ((int64_t)1 << 31)) return 0;
  return gmm_ws_layout(nullptr, n_frames_cap, K, D).bytes;
}

int air_gmm_prepare(const double* w, const double* mu, const double* var, int K, int D, double* params,
                    air_stream_t stream) {
  if (!gmm_shape_ok(K, D)) return AIR_EUNSUPPORTED;
  if (!w || !mu || !var || !params) return AIR_EINVAL;
  const int Kp = (K + 15) / 16 * 16;
  hipLaunchKernelGGL(gmm_prepare_kernel, dim3(Kp), dim3(kThreads), 0, air_stream(stream), w, mu, var, K, D, gmm_dp(D),
                     params);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

int air_gmm_accumulate(const float* x, int layout, int B, int Tcap, const int* n_frames, const double* params, int K,
                       int D, double* stats, void* ws, size_t ws_bytes, air_stream_t stream) {
  const int rc = gmm_check(x, layout, B, Tcap, params, K, D);
  if (rc != AIR_OK) return rc;
  if (!stats || !ws) return AIR_EINVAL;
  const int64_t n = (int64_t)B * Tcap;
  const GmmWs w = gmm_ws_layout(ws, n, K, D);
  if (ws_bytes < w.bytes) return AIR_EWORKSPACE;
  hipStream_t st = air_stream(stream);
  const int Dp = gmm_dp(D), KT = (K + 15) / 16, Kp = KT * 16;
  const Frames f{x, n_frames, layout, B, Tcap, D, Dp, n};
  const int rc2 = gmm_launch_lse(f, params, K, w.lse, w.ll_part, w.cnt_part, st);
  if (rc2 != AIR_OK) return rc2;
  const int64_t ntiles = gmm_tiles(n);
  const int nchunks = (int)gmm_chunks(ntiles, K);
  const size_t pd = gmm_partial_doubles(K, D);
  const dim3 grid((unsigned)nchunks, (unsigned)((KT + 3) / 4));
#define AIR_GMM_STATS(NJT) \
  hipLaunchKernelGGL((gmm_stats_kernel<NJT>), grid, dim3(kThreads), 0, st, f, params, KT, w.lse, ntiles, w.part, pd)
  switch (Dp) {
    case 8: AIR_GMM_STATS(1); break;
    case 32: AIR_GMM_STATS(4); break;
    case 64: AIR_GMM_STATS(8); break;
    default: AIR_GMM_STATS(16); break;
  }
#undef AIR_GMM_STATS
  AIR_CHECK_LAUNCH();
  const int total = K + 2 * K * D;
  hipLaunchKernelGGL(gmm_merge_kernel, dim3((total + kThreads - 1) / kThreads), dim3(kThreads), 0, st, w.part, pd, nchunks, K,
                     D, Dp, Kp, stats);
  AIR_CHECK_LAUNCH();
  hipLaunchKernelGGL(gmm_ll_merge_kernel, dim3(1), dim3(kThreads), 0, st, w.ll_part, w.cnt_part, ntiles, stats + total,
                     reinterpret_cast<long long*>(stats + total + 1));
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

int air_gmm_loglik(const float* x, int layout, int B, int Tcap, const int* n_frames, const double* params, int K, int D,
                   double* frame_ll, double* row_ll, void* ws, size_t ws_bytes, air_stream_t stream) {
  const int rc = gmm_check(x, layout, B, Tcap, params, K, D);
  if (rc != AIR_OK) return rc;
  if (!ws || (!frame_ll && !row_ll)) return AIR_EINVAL;
  const int64_t n = (int64_t)B * Tcap;
  const GmmWs w = gmm_ws_layout(ws, n, K, D);
  if (ws_bytes < w.bytes) return AIR_EWORKSPACE;
  hipStream_t st = air_stream(stream);
  const Frames f{x, n_frames, layout, B, Tcap, D, gmm_dp(D), n};
  double* lse = frame_ll ? frame_ll : w.lse;
  const int rc2 = gmm_launch_lse(f, params, K, lse, w.ll_part, w.cnt_part, st);
  if (rc2 != AIR_OK) return rc2;
  if (row_ll) {
    hipLaunchKernelGGL(gmm_row_mean_kernel, dim3(B), dim3(kThreads), 0, st, lse, Tcap, n_frames, row_ll);
    AIR_CHECK_LAUNCH();
  }
  return AIR_OK;
}

int air_debug_mfma_f64_probe(int nblocks, int iters, double* out, air_stream_t stream) {
  if (nblocks < 1 || nblocks > 65536 || iters < 1 || iters > (1 << 24) || !out) return AIR_EINVAL;
  hipLaunchKernelGGL(gmm_mfma_probe_kernel, dim3(nblocks), dim3(kThreads), 0, air_stream(stream), iters, out);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

int air_gmm_mstep(const double* stats, int K, int D, double reg_covar, double* w, double* mu, double* var,
                  double* lower_bound, air_stream_t stream) {
  if (!gmm_shape_ok(K, D)) return AIR_EUNSUPPORTED;
  if (!stats || !w || !mu || !var || !lower_bound || !(reg_covar >= 0.0)) return AIR_EINVAL;
  hipLaunchKernelGGL(gmm_mstep_kernel, dim3(K), dim3(kThreads), 0, air_stream(stream), stats, K, D, reg_covar, w, mu, var,
                     lower_bound);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

}  // extern "C"
