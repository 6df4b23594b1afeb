// RawBoost waveform augmentation (Tak et al., ICASSP 2022) on dense and ragged PCM batches: air_rawboost_design and
// air_rawboost_ragged.  include/air_hip.h ("RawBoost") is the arithmetic specification and the layout of the parameter
// table; this header is about how the work is cut.
//
// Launches of one call, back to back on the caller's stream, no host synchronisation, no atomics:
//   1. design   one workgroup per filter slot (6 per row): the notch cascade in fp64 - band filters, their linear
//               convolution, the 512-point response through a 1024-entry twiddle table, the gain - rounded once to fp32;
//   2. lnl      rows whose algorithm has the LnL stage: A = sum_i F(b_i, x^(i+1)), per-tile partial sums;
//   3. ssi      rows whose algorithm has the SSI stage: Q = F(b, n), n drawn in the kernel; per-tile partial sums of squares;
//   4. centre   LnL rows: A -= mean(A); per-tile partial max |A|;
//   5. - 7.     three pointwise passes.  Every one of them reads the row statistics the passes before it left (merged in
//               fp64 over the row's own tiles in ascending order), applies the pending peak rule or noise scale, and leaves
//               the partials the next one needs.  Which row finishes in which pass is listed in front of rb_point_kernel.
// A row's work is tiled by its own sample index alone (tile k = samples [2048 k, 2048 k + 2048)), every partial is a
// fixed-order reduction of one tile and the merge walks the row's tiles in order, so y[b, :L_b] carries the bits of the
// call on that utterance alone, and a call repeats its bits.
//
// The FIR (launches 2 and 3) is the direct form of the IR augmentation's fir_kernel (csrc/augment.hip): a workgroup owns
// 2048 outputs, a thread 8 consecutive ones; the x window of the tile (2048 + 512 samples) is staged ONCE in LDS in groups
// of 8 samples at a 48-byte stride; per 8 taps a thread slides a 16-sample register window by one group.  What is new is
// that the five filters of the Hammerstein sum share that window: the powers x^2 .. x^5 of a group are formed in registers
// as it is loaded (p_{j+1} = fl32(p_j x), 32 multiplies beside 320 FMAs), so one LDS read of x feeds five filters and
// the LDS holds one signal, not five.  The cascades have different lengths; they are staged at a common centre (tap k of
// a cascade of len taps sits at j = 256 - (len + 1) / 2 + k), zero elsewhere, and the loop runs over the union of their
// supports - a zero tap adds an exact zero, so the sum is the sum of the specification's terms in one fmaf chain.
// (Skipping, per group of 8 taps, the cascades that have only zeros there - a uniform branch - was measured: 10 % slower,
// the branch costs the unrolled FMA block more than the zeros do.)
//
// Measured at B = 64 x 64 000 (profiles/rawboost.md): the LnL launch runs at the rate of the unpacked fp32 FMA, which is
// what fir_kernel reached; the design launch is bound by the latency of its serial fp64 loops, not by arithmetic.
#include "air_common.h"
#include "air_pcm.h"
#include "air_philox.h"

namespace {

constexpr int RB_NT = 256, RB_R = 8, RB_T = RB_NT * RB_R;  // outputs per workgroup: the tile
constexpr int RB_MAXTAPS = 512;                            // per cascade; also the halo of a tile
constexpr int RB_NF = 5;                                   // filters of the LnL stage (slots 0 .. 4)
constexpr int RB_FILTERS = RB_NF + 1;                      // + the SSI filter (slot 5)
constexpr int RB_MAXBANDS = 8;
constexpr int RB_HDR = 8, RB_FREC = 2 + 3 * RB_MAXBANDS, RB_ROW = RB_HDR + RB_FILTERS * RB_FREC;  // doubles
constexpr int RB_GROUPS = (RB_T + RB_MAXTAPS) / 8;         // 320 groups of 8 staged samples
constexpr int RB_GS = 12;                                  // floats per group slot (8 data + 4 pad: see fir_kernel)
constexpr int RB_NSTAT = 6;                                // statistic slots per (row, tile)
constexpr int RB_MAXL = 1 << 20;                           // samples per row: what the host reserves per row in the ISD stream
enum { RB_S_SUM = 0, RB_S_CMAX = 1, RB_S_QSQ = 2, RB_S_P3 = 3, RB_S_P4 = 4 };
static_assert(RB_ROW == 164 && RB_GROUPS == 320, "the layout include/air_hip.h documents");

// the table is caller data: anything that is not one of the eight algorithms copies the row
__device__ __forceinline__ int rb_algo(const double* __restrict__ row) {
  const double a = row[0];
  return (a >= 0.0 && a <= 7.0) ? (int)a : -1;
}
__device__ __forceinline__ bool rb_has_lnl(int a) { return a == 0 || a == 3 || a == 4 || a == 5 || a == 7; }
__device__ __forceinline__ bool rb_has_isd(int a) { return a == 1 || a == 3 || a == 4 || a == 6 || a == 7; }
__device__ __forceinline__ bool rb_has_ssi(int a) { return a == 2 || a == 3 || a == 5 || a == 6; }

__device__ __forceinline__ double rb_wave_max_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// Sum / max of one value per thread over the workgroup (256 threads), in a fixed order: the butterfly inside a wave, the
// four waves in ascending order.  Every thread gets the result.  red: 4 doubles of LDS; two barriers.
__device__ __forceinline__ double rb_block_sum(double v, double* __restrict__ red) {
  v = air_wave_sum_d(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}
__device__ __forceinline__ double rb_block_max(double v, double* __restrict__ red) {
  v = rb_wave_max_d(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

// statistic `slot` of row b over its own tiles, ascending
__device__ __forceinline__ const double* rb_stat(const double* __restrict__ stats, int b, int slot, int ntcap) {
  return stats + ((size_t)b * RB_NSTAT + slot) * ntcap;
}
__device__ __forceinline__ double rb_merge_sum(const double* __restrict__ stats, int b, int slot, int ntcap, int L) {
  const double* __restrict__ p = rb_stat(stats, b, slot, ntcap);
  double s = 0.0;
  for (int k = 0; k < (L + RB_T - 1) / RB_T; ++k) s += p[k];
  return s;
}
__device__ __forceinline__ double rb_merge_max(const double* __restrict__ stats, int b, int slot, int ntcap, int L) {
  const double* __restrict__ p = rb_stat(stats, b, slot, ntcap);
  double s = 0.0;
  for (int k = 0; k < (L + RB_T - 1) / RB_T; ++k) s = fmax(s, p[k]);
  return s;
}

// four standard normals of one quad of the air_randn stream (air_philox.h), at scale 1
__device__ __forceinline__ void rb_randn_quad(uint64_t ctr, uint64_t key, float (&z)[4]) {
  uint32_t c[4];
  air_philox_block(ctr, key, c);
  air_philox_randn_quad(c, z);
}

// ISD, sample n of row b: selected iff word 0 < T; then v + g v (2 u1 - 1)(2 u2 - 1), every operation one fp32 rounding
__device__ __forceinline__ float rb_isd(float v, uint64_t ctr, uint64_t key, uint64_t T, float g) {
  uint32_t c[4];
  air_philox_block(ctr, key, c);
  if ((uint64_t)c[0] >= T) return v;
  const float a = 2.0f * air_philox_u01(c[1]) - 1.0f;
  const float d = 2.0f * air_philox_u01(c[2]) - 1.0f;
  return v + (g * v) * (a * d);
}

// ---- design ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double rb_sinc(double x) {  // numpy's sinc: sin(pi x) / (pi x)
  return x == 0.0 ? 1.0 : sinpi(x) / (3.141592653589793 * x);
}

// blockIdx.x = filter slot f = 6 b + s.  taps[f, 0:512] (zero behind len), lens[f]; a slot the row does not use, or one
// the call would refuse (even or out-of-range tap counts, more than 512 taps), gets len 0 and zero taps.
__global__ __launch_bounds__(RB_NT) void rb_design_kernel(const double* __restrict__ params, float* __restrict__ taps,
                                                          int* __restrict__ lens) {
  __shared__ double hb[RB_MAXTAPS];
  __shared__ double cas[2][RB_MAXTAPS];
  __shared__ double twc[1024], tws[1024];
  __shared__ double red[4];
  const int f = blockIdx.x, t = threadIdx.x;
  const double* __restrict__ row = params + (size_t)(f / RB_FILTERS) * RB_ROW;
  const double* __restrict__ rec = row + RB_HDR + (f % RB_FILTERS) * RB_FREC;
  float* __restrict__ out = taps + (size_t)f * RB_MAXTAPS;
  const double nbd = rec[1];
  const int nb = (nbd >= 1.0 && nbd <= (double)RB_MAXBANDS) ? (int)nbd : 0;
  bool ok = nb > 0 && rb_algo(row) >= 0;
  int len = 1;
  for (int k = 0; k < nb; ++k) {
    const double cd = rec[2 + 3 * k + 2];
    const int c = (cd >= 1.0 && cd <= (double)RB_MAXTAPS) ? (int)cd : 0;
    if (!(c & 1)) ok = false;
    len += c - 1;
  }
  if (!ok || len < 1 || len > RB_MAXTAPS) {  // (uniform over the workgroup)
    for (int n = t; n < RB_MAXTAPS; n += RB_NT) out[n] = 0.0f;
    if (t == 0) lens[f] = 0;
    return;
  }
  for (int j = t; j < 1024; j += RB_NT) {  // e^(i pi j / 512)
    double s, c;
    sincospi((double)j / 512.0, &s, &c);
    twc[j] = c;
    tws[j] = s;
  }
  if (t == 0) cas[0][0] = 1.0;
  int cur = 0, clen = 1;
  for (int k = 0; k < nb; ++k) {
    const double fc = rec[2 + 3 * k], bw = rec[2 + 3 * k + 1];
    const int c = (int)rec[2 + 3 * k + 2];
    double f1 = fc - bw / 2.0, f2 = fc + bw / 2.0;
    if (!(f1 > 0.0)) f1 = 1.0 / 1000.0;
    if (!(f2 < 8000.0)) f2 = 8000.0 - 1.0 / 1000.0;
    const double l = f1 / 8000.0, r = f2 / 8000.0;
    __syncthreads();  // hb and cas[cur ^ 1] were last read by the band before
    for (int m = t; m < c; m += RB_NT) {
      const double x = (double)m - (double)(c - 1) / 2.0;
      const double h = l * rb_sinc(l * x) + rb_sinc(x) - r * rb_sinc(r * x);
      const double w = c == 1 ? 1.0 : 0.54 - 0.46 * cospi(2.0 * (double)m / (double)(c - 1));
      hb[m] = h * w;
    }
    __syncthreads();
    double s = 0.0;
#pragma unroll 8
    for (int m = 0; m < c; ++m) s += hb[m];  // every thread the same sum, in index order
    __syncthreads();
    for (int m = t; m < c; m += RB_NT) hb[m] /= s;
    __syncthreads();
    for (int n = t; n < clen + c - 1; n += RB_NT) {
      double acc = 0.0;
#pragma unroll 8
      for (int j = max(0, n - clen + 1); j <= min(c - 1, n); ++j) acc += hb[j] * cas[cur][n - j];
      cas[cur ^ 1][n] = acc;
    }
    cur ^= 1;
    clen += c - 1;
  }
  __syncthreads();
  const double* __restrict__ bq = cas[cur];
  double peak = 0.0;
  for (int k = t; k < 512; k += RB_NT) {  // |H(k pi / 512)|
    double re = 0.0, im = 0.0;
#pragma unroll 8
    for (int n = 0; n < clen; ++n) {
      const int j = (k * n) & 1023;
      re += bq[n] * twc[j];
      im -= bq[n] * tws[j];
    }
    peak = fmax(peak, sqrt(re * re + im * im));
  }
  peak = rb_block_max(peak, red);
  const double gain = pow(10.0, rec[0] / 20.0) / peak;
  for (int n = t; n < RB_MAXTAPS; n += RB_NT) out[n] = n < clen ? (float)(bq[n] * gain) : 0.0f;
  if (t == 0) lens[f] = clen;
}

// ---- the FIR core ------------------------------------------------------------------------------------------------------
// group g of the staged window into registers, with its powers: w[s] = x^(s + 1), formed in fp32 in this order
template <int NS>
__device__ __forceinline__ void rb_load_group(const float* __restrict__ xs, int g, float (&w)[NS][8]) {
  const float4* p = reinterpret_cast<const float4*>(xs + g * RB_GS);
  const float4 a = p[0], c = p[1];
  w[0][0] = a.x; w[0][1] = a.y; w[0][2] = a.z; w[0][3] = a.w;
  w[0][4] = c.x; w[0][5] = c.y; w[0][6] = c.z; w[0][7] = c.w;
#pragma unroll
  for (int s = 1; s < NS; ++s)
#pragma unroll
    for (int i = 0; i < 8; ++i) w[s][i] = w[s - 1][i] * w[0][i];
}

// out[r] = sum_s sum_j hs[s][j] p_s[n + 256 - j], n = n0 + 8 t + r, j in [8 jb_lo, 8 jb_hi); staged position p of xs is
// sample n0 - 255 + p.  Thread t, taps 8 jb + i: position 8 (t + 63 - jb) + (r - i + 7).
template <int NS>
__device__ __forceinline__ void rb_fir_core(const float* __restrict__ xs, const float* __restrict__ hs, int jb_lo, int jb_hi,
                                            int t, float (&out)[RB_R]) {
  float wlo[NS][8], whi[NS][8];
#pragma unroll
  for (int r = 0; r < RB_R; ++r) out[r] = 0.0f;
  if (jb_lo >= jb_hi) return;
  rb_load_group<NS>(xs, t + 64 - jb_lo, whi);
  for (int jb = jb_lo; jb < jb_hi; ++jb) {
    rb_load_group<NS>(xs, t + 63 - jb, wlo);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const float4 h0 = reinterpret_cast<const float4*>(hs + s * RB_MAXTAPS + jb * 8)[0];
      const float4 h1 = reinterpret_cast<const float4*>(hs + s * RB_MAXTAPS + jb * 8)[1];
      const float h[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int r = 0; r < RB_R; ++r) {
          const int w = r - i + 7;  // 0..14 within [wlo | whi]
          out[r] = fmaf(h[i], w < 8 ? wlo[s][w] : whi[s][w - 8], out[r]);
        }
    }
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int i = 0; i < 8; ++i) whi[s][i] = wlo[s][i];
  }
}

// Stage NS cascades of row b (slots slot0 ..) at their common centre; returns the union of their supports in groups of 8.
template <int NS>
__device__ __forceinline__ void rb_stage_taps(const float* __restrict__ taps, const int* __restrict__ lens, int b, int slot0,
                                              float* __restrict__ hs, int t, int& jb_lo, int& jb_hi) {
  int jlo = RB_MAXTAPS, jhi = 0;
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int f = b * RB_FILTERS + slot0 + s;
    const int len = min(max(lens[f], 0), RB_MAXTAPS);
    const int sh = RB_MAXTAPS / 2 - (len + 1) / 2;
    const float* __restrict__ hb = taps + (size_t)f * RB_MAXTAPS;
    for (int j = t; j < RB_MAXTAPS; j += RB_NT) hs[s * RB_MAXTAPS + j] = (j >= sh && j < sh + len) ? hb[j - sh] : 0.0f;
    if (len > 0) {
      jlo = min(jlo, sh);
      jhi = max(jhi, sh + len);
    }
  }
  jb_lo = jlo >> 3;
  jb_hi = jhi > 0 ? (jhi + 7) >> 3 : 0;
}

// LnL: A[b, n] = sum_i F(b_i, x^(i+1))[n], n < L_b; stats slot RB_S_SUM = the tile's sum
template <typename T>
__global__ __launch_bounds__(RB_NT) void rb_lnl_kernel(const T* __restrict__ x, int Lcap, const int* __restrict__ lengths,
                                                       const double* __restrict__ params, const float* __restrict__ taps,
                                                       const int* __restrict__ lens, float* __restrict__ A,
                                                       double* __restrict__ stats, int ntcap) {
  __shared__ __attribute__((aligned(16))) float xs[RB_GROUPS * RB_GS];
  __shared__ __attribute__((aligned(16))) float hs[RB_NF * RB_MAXTAPS];
  __shared__ double red[4];
  const int b = blockIdx.y, n0 = blockIdx.x * RB_T, t = threadIdx.x;
  const int L = air_row_len(lengths, b, Lcap);
  if (!rb_has_lnl(rb_algo(params + (size_t)b * RB_ROW)) || n0 >= L) return;
  const T* __restrict__ xb = x + (size_t)b * Lcap;
  int jb_lo, jb_hi;
  rb_stage_taps<RB_NF>(taps, lens, b, 0, hs, t, jb_lo, jb_hi);
  for (int p = t; p < RB_GROUPS * 8; p += RB_NT) {
    const int m = n0 - (RB_MAXTAPS / 2 - 1) + p;
    xs[(p >> 3) * RB_GS + (p & 7)] = (m >= 0 && m < L) ? air_pcm_sample(xb, m) : 0.0f;
  }
  __syncthreads();
  float out[RB_R];
  rb_fir_core<RB_NF>(xs, hs, jb_lo, jb_hi, t, out);
  float* __restrict__ ab = A + (size_t)b * Lcap;
  double s = 0.0;
#pragma unroll
  for (int r = 0; r < RB_R; ++r) {
    const int n = n0 + t * RB_R + r;
    if (n < L) {
      ab[n] = out[r];
      s += (double)out[r];
    }
  }
  s = rb_block_sum(s, red);
  if (t == 0) stats[((size_t)b * RB_NSTAT + RB_S_SUM) * ntcap + blockIdx.x] = s;
}

// SSI: Q[b, n] = F(b_ssi, noise)[n], n < L_b, noise[m] = element m of the randn stream at quad offset ssi_base + b ceil(Lcap / 4);
// stats slot RB_S_QSQ = the tile's sum of squares
__global__ __launch_bounds__(RB_NT) void rb_ssi_kernel(int Lcap, const int* __restrict__ lengths, const double* __restrict__ params,
                                                       const float* __restrict__ taps, const int* __restrict__ lens,
                                                       float* __restrict__ Q, double* __restrict__ stats, int ntcap) {
  __shared__ __attribute__((aligned(16))) float xs[RB_GROUPS * RB_GS];
  __shared__ __attribute__((aligned(16))) float hs[RB_MAXTAPS];
  __shared__ double red[4];
  const int b = blockIdx.y, n0 = blockIdx.x * RB_T, t = threadIdx.x;
  const int L = air_row_len(lengths, b, Lcap);
  const double* __restrict__ row = params + (size_t)b * RB_ROW;
  if (!rb_has_ssi(rb_algo(row)) || n0 >= L) return;
  int jb_lo, jb_hi;
  rb_stage_taps<1>(taps, lens, b, RB_NF, hs, t, jb_lo, jb_hi);
  const uint64_t base = (uint64_t)row[4] + (uint64_t)b * (uint64_t)((Lcap + 3) / 4), key = (uint64_t)row[7];
  const int m0 = n0 - (RB_MAXTAPS / 2 - 1);         // sample of staged position 0; >= -255
  const int mq0 = ((m0 + 256) & ~3) - 256;          // the multiple of 4 at or below it
  for (int qi = t; qi < RB_GROUPS * 2 + 1; qi += RB_NT) {
    const int m = mq0 + 4 * qi;
    float z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (m >= 0 && m < L) rb_randn_quad(base + (uint64_t)(m >> 2), key, z);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int p = m + e - m0;
      if (p >= 0 && p < RB_GROUPS * 8) xs[(p >> 3) * RB_GS + (p & 7)] = (m + e >= 0 && m + e < L) ? z[e] : 0.0f;
    }
  }
  __syncthreads();
  float out[RB_R];
  rb_fir_core<1>(xs, hs, jb_lo, jb_hi, t, out);
  float* __restrict__ qb = Q + (size_t)b * Lcap;
  double s = 0.0;
#pragma unroll
  for (int r = 0; r < RB_R; ++r) {
    const int n = n0 + t * RB_R + r;
    if (n < L) {
      qb[n] = out[r];
      s += (double)out[r] * (double)out[r];
    }
  }
  s = rb_block_sum(s, red);
  if (t == 0) stats[((size_t)b * RB_NSTAT + RB_S_QSQ) * ntcap + blockIdx.x] = s;
}

// LnL rows: A -= (float)(sum A / L); stats slot RB_S_CMAX = the tile's max |A|
__global__ __launch_bounds__(RB_NT) void rb_centre_kernel(int Lcap, const int* __restrict__ lengths, const double* __restrict__ params,
                                                          float* __restrict__ A, double* __restrict__ stats, int ntcap) {
  __shared__ double red[4];
  const int b = blockIdx.y, n0 = blockIdx.x * RB_T, t = threadIdx.x;
  const int L = air_row_len(lengths, b, Lcap);
  if (!rb_has_lnl(rb_algo(params + (size_t)b * RB_ROW)) || n0 >= L) return;
  const float mu = (float)(rb_merge_sum(stats, b, RB_S_SUM, ntcap, L) / (double)L);
  float* __restrict__ ab = A + (size_t)b * Lcap;
  float peak = 0.0f;
  for (int n = n0 + t; n < min(n0 + RB_T, L); n += RB_NT) {
    const float v = ab[n] - mu;
    ab[n] = v;
    peak = fmaxf(peak, fabsf(v));
  }
  const double m = rb_block_max((double)peak, red);
  if (t == 0) stats[((size_t)b * RB_NSTAT + RB_S_CMAX) * ntcap + blockIdx.x] = m;
}

// N0 with the row peak: v / peak if peak > 1
__device__ __forceinline__ float rb_n0(float v, float peak) { return peak > 1.0f ? v / peak : v; }

// SSI scale ||v|| / (||q|| 10^(SNR / 20)) in fp64, rounded once; 0 when ||q|| = 0
__device__ __forceinline__ float rb_ssi_scale(double vsq, double qsq, double snr) {
  return qsq > 0.0 ? (float)(sqrt(vsq) / (sqrt(qsq) * pow(10.0, snr / 20.0))) : 0.0f;
}

// The pointwise passes.  W is the "current signal" of a row between passes.  Per algorithm (n < L_b):
//   pass 0   every row: y[n >= L_b] = 0.  -1: y = x.  0: y = N0(A) - done.  5: W = N0(A), |W|^2.  2: W = x, |W|^2.
//            3, 4: W = isd(N0(A)), max |W|.  1, 6, 7: W = isd(x), max |W|.                     -> slot RB_S_P3
//   pass 1   1, 4: y = N0(W) - done.  3, 6: W = N0(W), |W|^2.  7: W = N0(A) + N0(W), max |W|.  -> slot RB_S_P4
//            2, 5: y = W + Q scale(P3, QSQ) - done.
//   pass 2   3, 6: y = W + Q scale(P4, QSQ).  7: y = N0(W).
template <typename T>
__global__ __launch_bounds__(RB_NT) void rb_point_kernel(int pass, const T* __restrict__ x, int Lcap, const int* __restrict__ lengths,
                                                         const double* __restrict__ params, const float* __restrict__ A,
                                                         float* __restrict__ W, const float* __restrict__ Q, float* __restrict__ y,
                                                         double* __restrict__ stats, int ntcap) {
  __shared__ double red[4];
  const int b = blockIdx.y, n0 = blockIdx.x * RB_T, t = threadIdx.x;
  const int L = air_row_len(lengths, b, Lcap);
  const double* __restrict__ row = params + (size_t)b * RB_ROW;
  const int a = rb_algo(row);
  const T* __restrict__ xb = x + (size_t)b * Lcap;
  const float* __restrict__ ab = A + (size_t)b * Lcap;
  const float* __restrict__ qb = Q + (size_t)b * Lcap;
  float* __restrict__ wb = W + (size_t)b * Lcap;
  float* __restrict__ yb = y + (size_t)b * Lcap;
  const int nend = min(n0 + RB_T, L);  // this tile's live samples: [n0, nend)
  if (pass == 0) {
    for (int n = max(n0, L) + t; n < min(n0 + RB_T, Lcap); n += RB_NT) yb[n] = 0.0f;  // (max(n0, L) + t: the tail only)
    if (a < 0) {
      for (int n = n0 + t; n < nend; n += RB_NT) yb[n] = air_pcm_sample(xb, n);
      return;
    }
  }
  if (a < 0 || n0 >= L) return;
  const bool lnl = rb_has_lnl(a);
  // (every condition below is uniform over the workgroup)
  double stat = 0.0;
  bool want_sum = false, want_max = false;
  if (pass == 0) {
    const float pk = lnl ? (float)rb_merge_max(stats, b, RB_S_CMAX, ntcap, L) : 0.0f;
    if (a == 0) {
      for (int n = n0 + t; n < nend; n += RB_NT) yb[n] = rb_n0(ab[n], pk);
    } else if (a == 5 || a == 2) {
      for (int n = n0 + t; n < nend; n += RB_NT) {
        const float v = a == 5 ? rb_n0(ab[n], pk) : air_pcm_sample(xb, n);
        wb[n] = v;
        stat += (double)v * (double)v;
      }
      want_sum = true;
    } else {  // the ISD stage, on N0(LnL(x)) for 3 and 4, on x for 1, 6 and 7
      const uint64_t T64 = (uint64_t)row[1], key = (uint64_t)row[6];
      const uint64_t base = (uint64_t)row[3] + (uint64_t)b * (uint64_t)Lcap;
      const float g = (float)row[2];
      const bool chained = a == 3 || a == 4;
      float peak = 0.0f;
      for (int n = n0 + t; n < nend; n += RB_NT) {
        const float v = chained ? rb_n0(ab[n], pk) : air_pcm_sample(xb, n);
        const float w = rb_isd(v, base + (uint64_t)n, key, T64, g);
        wb[n] = w;
        peak = fmaxf(peak, fabsf(w));
      }
      stat = (double)peak;
      want_max = true;
    }
  } else if (pass == 1) {
    if (a == 0) return;
    if (a == 2 || a == 5) {
      const float sc = rb_ssi_scale(rb_merge_sum(stats, b, RB_S_P3, ntcap, L), rb_merge_sum(stats, b, RB_S_QSQ, ntcap, L), row[5]);
      for (int n = n0 + t; n < nend; n += RB_NT) yb[n] = fmaf(qb[n], sc, wb[n]);
      return;
    }
    const float pk = (float)rb_merge_max(stats, b, RB_S_P3, ntcap, L);
    if (a == 1 || a == 4) {
      for (int n = n0 + t; n < nend; n += RB_NT) yb[n] = rb_n0(wb[n], pk);
    } else if (a == 3 || a == 6) {
      for (int n = n0 + t; n < nend; n += RB_NT) {
        const float v = rb_n0(wb[n], pk);
        wb[n] = v;
        stat += (double)v * (double)v;
      }
      want_sum = true;
    } else {  // 7
      const float pa = (float)rb_merge_max(stats, b, RB_S_CMAX, ntcap, L);
      float peak = 0.0f;
      for (int n = n0 + t; n < nend; n += RB_NT) {
        const float v = rb_n0(ab[n], pa) + rb_n0(wb[n], pk);
        wb[n] = v;
        peak = fmaxf(peak, fabsf(v));
      }
      stat = (double)peak;
      want_max = true;
    }
  } else {
    if (a == 3 || a == 6) {
      const float sc = rb_ssi_scale(rb_merge_sum(stats, b, RB_S_P4, ntcap, L), rb_merge_sum(stats, b, RB_S_QSQ, ntcap, L), row[5]);
      for (int n = n0 + t; n < nend; n += RB_NT) yb[n] = fmaf(qb[n], sc, wb[n]);
    } else if (a == 7) {
      const float pk = (float)rb_merge_max(stats, b, RB_S_P4, ntcap, L);
      for (int n = n0 + t; n < nend; n += RB_NT) yb[n] = rb_n0(wb[n], pk);
    }
    return;
  }
  if (want_sum || want_max) {
    const double v = want_sum ? rb_block_sum(stat, red) : rb_block_max(stat, red);
    if (t == 0) stats[((size_t)b * RB_NSTAT + (pass == 0 ? RB_S_P3 : RB_S_P4)) * ntcap + blockIdx.x] = v;
  }
}

inline size_t rb_align(size_t v) { return (v + 255) & ~(size_t)255; }

struct RbPlan {  // the workspace of one call
  int ntcap;
  size_t off_lens, off_stats, off_A, off_W, off_Q, total;
};

inline RbPlan rb_plan(int B, int Lcap) {
  RbPlan g;
  g.ntcap = (Lcap + RB_T - 1) / RB_T;
  const size_t buf = rb_align((size_t)B * Lcap * sizeof(float));
  g.off_lens = rb_align((size_t)B * RB_FILTERS * RB_MAXTAPS * sizeof(float));
  g.off_stats = g.off_lens + rb_align((size_t)B * RB_FILTERS * sizeof(int));
  g.off_A = g.off_stats + rb_align((size_t)B * RB_NSTAT * g.ntcap * sizeof(double));
  g.off_W = g.off_A + buf;
  g.off_Q = g.off_W + buf;
  g.total = g.off_Q + buf;
  return g;
}

template <typename T>
int rb_launch(const T* x, int B, int Lcap, const int* lengths, const double* params, float* y, void* ws, hipStream_t st) {
  const RbPlan g = rb_plan(B, Lcap);
  char* base = reinterpret_cast<char*>(ws);
  float* taps = reinterpret_cast<float*>(base);
  int* lens = reinterpret_cast<int*>(base + g.off_lens);
  double* stats = reinterpret_cast<double*>(base + g.off_stats);
  float* A = reinterpret_cast<float*>(base + g.off_A);
  float* W = reinterpret_cast<float*>(base + g.off_W);
  float* Q = reinterpret_cast<float*>(base + g.off_Q);
  const dim3 grid(g.ntcap, B), block(RB_NT);
  hipLaunchKernelGGL(rb_design_kernel, dim3(B * RB_FILTERS), block, 0, st, params, taps, lens);
  AIR_CHECK_LAUNCH();
  hipLaunchKernelGGL(rb_lnl_kernel<T>, grid, block, 0, st, x, Lcap, lengths, params, taps, lens, A, stats, g.ntcap);
  AIR_CHECK_LAUNCH();
  hipLaunchKernelGGL(rb_ssi_kernel, grid, block, 0, st, Lcap, lengths, params, taps, lens, Q, stats, g.ntcap);
  AIR_CHECK_LAUNCH();
  hipLaunchKernelGGL(rb_centre_kernel, grid, block, 0, st, Lcap, lengths, params, A, stats, g.ntcap);
  AIR_CHECK_LAUNCH();
  for (int pass = 0; pass < 3; ++pass) {
    hipLaunchKernelGGL(rb_point_kernel<T>, grid, block, 0, st, pass, x, Lcap, lengths, params, A, W, Q, y, stats, g.ntcap);
    AIR_CHECK_LAUNCH();
  }
  return AIR_OK;
}

}  // namespace

extern "C" {

int air_rawboost_tile(void) { return RB_T; }

int air_rawboost_row_doubles(void) { return RB_ROW; }

size_t air_rawboost_ws_bytes(int B, int Lcap) {
  if (B <= 0 || B > 65535 || Lcap <= 0 || Lcap > RB_MAXL) return 0;
  return rb_plan(B, Lcap).total;
}

int air_rawboost_design(const double* params, int B, float* taps, int* lens, air_stream_t stream) {
  if (!params || !taps || !lens || B <= 0 || B > 65535) return AIR_EINVAL;
  hipLaunchKernelGGL(rb_design_kernel, dim3(B * RB_FILTERS), dim3(RB_NT), 0, air_stream(stream), params, taps, lens);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

int air_rawboost_ragged(const float* x, const int16_t* x16, int B, int Lcap, const int* lengths_dev_or_null, const double* params,
                        float* y, void* ws, size_t ws_bytes, air_stream_t stream) {
  if ((x != nullptr) == (x16 != nullptr) || !y || !params || B <= 0 || B > 65535 || Lcap <= 0 || Lcap > RB_MAXL || (x && x == y))
    return AIR_EINVAL;
  if (!ws || ws_bytes < air_rawboost_ws_bytes(B, Lcap)) return AIR_EWORKSPACE;
  hipStream_t st = air_stream(stream);
  if (x16) return rb_launch(reinterpret_cast<const short*>(x16), B, Lcap, lengths_dev_or_null, params, y, ws, st);
  return rb_launch(x, B, Lcap, lengths_dev_or_null, params, y, ws, st);
}

}  // extern "C"
