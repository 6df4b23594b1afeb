// CQCC front-end for gfx950: constant-Q cepstral coefficients from PCM, defined by the formulas of include/air_hip.h
// ("CQCC front-end"; tests/cqcc_oracle.py restates them in numpy fp64).  Three pieces of work, five kernels:
//
//   pyramid   level s + 1 = the 47-tap Kaiser half-band low-pass of level s, decimated by two (one launch per level, a
//             thread per output sample, the taps in index order).  Octaves 0 and 1 read the row itself, octave o >= 2
//             reads level o - 1, so every analysed band but the top one lies in [R/8, R/4) of its own rate R and all
//             of them share ONE atom table; the top octave's, at [R/4, R/2), is the second.
//   product   per (row, octave, 64 frames): X[frame][bin] = sum_n x[c_frame + n - H] * atom[n][bin] as a dense
//             (64 x KP) x (KP x 192) product on v_mfma_f32_32x32x2_f32, KP = 2 H + 1 rounded up to 32 (1120 for the
//             shared table, 576 for the top octave's).  The 192 columns are the real and imaginary parts of 96 bins.
//             The A operand is never formed: the workgroup stages the stretch of the level its 64 overlapping frames
//             span (at most 63 * hop + KP = 11 200 floats) once, and lane (frame i, k) reads s_x[c_i - c_0 + k].  The
//             atom table streams through LDS in 32-row chunks (24 KB), prefetched into registers under the MFMAs of
//             the chunk before.  4 waves = 2 frame halves x 2 column halves; a wave holds 3 accumulators of 32 x 32
//             (48 AGPR-able registers).  Epilogue: |X|^2 by one cross-lane add (a column block holds 16 real parts
//             and the 16 imaginary parts of the same bins), log(|X|^2 + eps), stored to the (B, T, K) log spectrum.
//   tail      statics c[t][q] = sum_k P[q][k] S[t][k] in k order (P: the fused interpolation x DCT-II matrix of the
//             plan), then delta / delta-delta over the row's own frames and the copy-out in either layout.
//
// The (B, T, K) log spectrum is kept in the workspace: at 64 x 401 x 864 it is 89 MB written once and read once, about
// 45 us of HBM time beside a product of 1e11 flop ("CQCC front-end").
//
// LDS of the product kernel: 44 800 B of stretch + 24 576 B of atom chunk = 69 376 B: two workgroups per CU of 160 KB, so
// one workgroup's barriers and chunk stores hide under the other's MFMAs.
//
// Every sum runs in a fixed order, nothing is atomic, a frame's arithmetic does not depend on the batch it is in (so a
// ragged row equals the dense call on it alone, bit for bit), and no sample at or beyond a row's length is read.
#include <math.h>
#include <string.h>

#include "air_common.h"
#include "air_pcm.h"

namespace {

constexpr int NBIN = 96;            // bins per octave (the only geometry built)
constexpr int NCOL = 2 * NBIN;      // columns of an atom table: real and imaginary parts
constexpr int MAXO = 9;             // octaves
constexpr int MAXQ = 32;            // cepstral coefficients
constexpr int MAXK = NBIN * MAXO;   // 864
constexpr int MAXJ = 64;            // pyramid taps held by the plan
constexpr int FIR_J = 47;           // taps of the half-band low-pass
constexpr double FIR_BETA = 16.0;   // its Kaiser beta
constexpr int KP0 = 576;            // rows of the top octave's table (2 * 275 + 1 = 551 live)
constexpr int KP1 = 1120;           // rows of the shared table (2 * 551 + 1 = 1103 live)
constexpr int KC = 32;              // rows of a staged chunk
constexpr int FT = 64;              // frames per workgroup of the product kernel
constexpr int NT = 256;             // its threads
constexpr int MAXHOP = 160;
constexpr int SX = 63 * MAXHOP + KP1;  // 11,200 staged samples at most
constexpr int CQCC_MAGIC = 0x43514343;
constexpr double CQ_PI = 3.14159265358979323846;

using f32x16 = __attribute__((ext_vector_type(16))) float;

struct CqccPlan {
  int magic, O, hop, n_coef, K, J, H0, H1;
  int d, M, pad0, pad1;
  float eps, padf[3];
  float h[MAXJ];
  float proj[MAXQ * MAXK];                                   // [q][k]
  __attribute__((aligned(16))) float atoms0[KP0 * NCOL];     // [row][column], the top octave
  __attribute__((aligned(16))) float atoms1[KP1 * NCOL];     // every other octave
};

struct CqccArgs {
  const float* pcm;
  const short* pcm16;
  const CqccPlan* plan;
  const int* lengths;   // null: every row holds Lcap samples
  const int* start;
  float* levels;        // pyramid levels 1 .. O - 2
  float* spec;          // (B, Tcap, K) log power
  float* stat;          // (B, Tcap, n_coef)
  float* out;
  long lvl_off[MAXO];   // first float of level s in `levels`
  int lvl_len[MAXO];    // row stride of level s = ceil(Lcap / 2^s)
  int B, Lcap, Tcap, O, hop, n_coef, K, feat_len, pad_mode;
};

// column q of a table <-> (bin, part): blocks of 32 columns hold 16 real parts, then the same bins' imaginary parts
__host__ __device__ constexpr int atom_col(int bin, int part) { return (bin >> 4) * 32 + part * 16 + (bin & 15); }

__device__ __forceinline__ bool plan_ok(const CqccPlan* p, const CqccArgs& a) {
  return p->magic == CQCC_MAGIC && p->O == a.O && p->hop == a.hop && p->n_coef == a.n_coef;
}

// ---- pyramid: level s -> s + 1 ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cqcc_pyramid(CqccArgs a, int s) {
  const CqccPlan* __restrict__ plan = a.plan;
  if (!plan_ok(plan, a)) return;
  const int b = blockIdx.y;
  const int n = blockIdx.x * 256 + threadIdx.x;
  const int L = air_row_len(a.lengths, b, a.Lcap);
  const int Lin = (int)(((long)L + (1L << s) - 1) >> s);
  const int Lout = (Lin + 1) >> 1;
  if (n >= Lout) return;
  const int J = plan->J, half = (J - 1) / 2;
  const float* __restrict__ in = s == 0 ? nullptr : a.levels + a.lvl_off[s] + (size_t)b * a.lvl_len[s];
  const float* __restrict__ row = a.pcm ? a.pcm + (size_t)b * a.Lcap : nullptr;
  const short* __restrict__ row16 = a.pcm16 ? a.pcm16 + (size_t)b * a.Lcap : nullptr;
  float acc = 0.0f;
  for (int j = 0; j < J; ++j) {
    const int idx = 2 * n + j - half;
    if (idx < 0 || idx >= Lin) continue;
    const float x = s == 0 ? (row16 ? air_pcm_sample(row16, idx) : row[idx]) : in[idx];
    acc = fmaf(plan->h[j], x, acc);
  }
  a.levels[a.lvl_off[s + 1] + (size_t)b * a.lvl_len[s + 1] + n] = acc;
}

// ---- per-octave product -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT, 2) void cqcc_product(CqccArgs a) {
  __shared__ __attribute__((aligned(16))) float s_x[SX];
  __shared__ __attribute__((aligned(16))) float s_b[KC * NCOL];

  const CqccPlan* __restrict__ plan = a.plan;
  if (!plan_ok(plan, a)) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tile = blockIdx.x, o = blockIdx.y, b = blockIdx.z;
  const int hop = a.hop;
  const int L = air_row_len(a.lengths, b, a.Lcap);
  const int T = 1 + L / hop;
  const int t0 = tile * FT;
  if (t0 >= T) return;  // (workgroup-uniform, ahead of every barrier)
  const int s = o < 2 ? 0 : o - 1;
  const int Ls = (int)(((long)L + (1L << s) - 1) >> s);
  const float* __restrict__ atoms = o == 0 ? plan->atoms0 : plan->atoms1;
  const int H = o == 0 ? plan->H0 : plan->H1;
  const int KP = o == 0 ? KP0 : KP1;
  const int tl = min(t0 + FT - 1, T - 1);
  const int c0 = (int)(((long)t0 * hop) >> s);
  const int cl = (int)(((long)tl * hop) >> s);

  // the stretch of the level that frames t0 .. tl read, zeros outside the row's own samples
  {
    const int base = c0 - H;
    const int count = min(cl - c0 + KP, SX);
    const float* __restrict__ lvl = s == 0 ? nullptr : a.levels + a.lvl_off[s] + (size_t)b * a.lvl_len[s];
    const float* __restrict__ row = a.pcm ? a.pcm + (size_t)b * a.Lcap : nullptr;
    const short* __restrict__ row16 = a.pcm16 ? a.pcm16 + (size_t)b * a.Lcap : nullptr;
    for (int j = tid; j < count; j += NT) {
      const int idx = base + j;
      float v = 0.0f;
      if (idx >= 0 && idx < Ls) v = s == 0 ? (row16 ? air_pcm_sample(row16, idx) : row[idx]) : lvl[idx];
      s_x[j] = v;
    }
  }

  const int mh = wave & 1, nh = wave >> 1;
  const int kk = lane >> 5;
  const int fi = min(t0 + mh * 32 + (lane & 31), tl);  // frames behind the row's last compute it again, unstored
  const int coff = (int)(((long)fi * hop) >> s) - c0;
  const float* __restrict__ xa = s_x + coff + kk;
  const float* __restrict__ bb = s_b + kk * NCOL + nh * 96 + (lane & 31);

  f32x16 acc[3];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[c][r] = 0.0f;

  constexpr int NV = KC * NCOL / 4 / NT;  // 6 float4 per thread and chunk
  float4 pre[NV];
  auto fetch = [&](int ch) {
    const float4* __restrict__ src = reinterpret_cast<const float4*>(atoms + (size_t)ch * KC * NCOL);
#pragma unroll
    for (int q = 0; q < NV; ++q) pre[q] = src[tid + q * NT];
  };
  const int nchunks = KP / KC;
  fetch(0);
  for (int ch = 0; ch < nchunks; ++ch) {
    __syncthreads();  // the chunk before is consumed (first trip: the stretch is staged)
#pragma unroll
    for (int q = 0; q < NV; ++q) reinterpret_cast<float4*>(s_b)[tid + q * NT] = pre[q];
    __syncthreads();
    if (ch + 1 < nchunks) fetch(ch + 1);
    const float* __restrict__ xk = xa + ch * KC;
#pragma unroll
    for (int ks = 0; ks < KC / 2; ++ks) {
      const float av = xk[2 * ks];
#pragma unroll
      for (int c = 0; c < 3; ++c)
        acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bb[2 * ks * NCOL + c * 32], acc[c], 0, 0, 0);
    }
  }

  // |X|^2 = re^2 + im^2 (lane j and lane j + 16 of a column block), log, store
  const float eps = plan->eps;
  const int K = a.K;
  const int kbase = (a.O - 1 - o) * NBIN + nh * 48 + (lane & 15);
  float* __restrict__ srow = a.spec + (size_t)b * a.Tcap * K;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float p = acc[c][r] * acc[c][r];
      const float q = __shfl_xor(p, 16, 64);
      const float pw = (lane & 16) ? q + p : p + q;  // re^2 + im^2 in that order on every lane
      const int t = t0 + mh * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      if ((lane & 16) == 0 && t <= tl) srow[(size_t)t * K + kbase + c * 16] = logf(pw + eps);
    }
  }
}

// ---- statics: c[t][q] = sum_k P[q][k] S[t][k] -----------------------------------------------------------------------
__global__ __launch_bounds__(256) void cqcc_project(CqccArgs a) {
  const CqccPlan* __restrict__ plan = a.plan;
  if (!plan_ok(plan, a)) return;
  const int b = blockIdx.y;
  const int q = threadIdx.x & 31;
  const int tg = blockIdx.x * 32 + (threadIdx.x >> 5) * 4;
  const int L = air_row_len(a.lengths, b, a.Lcap);
  const int T = 1 + L / a.hop;
  if (q >= a.n_coef || tg >= T) return;
  const int K = a.K;
  const float4* __restrict__ pr = reinterpret_cast<const float4*>(plan->proj + (size_t)q * K);
  const float* __restrict__ sb = a.spec + (size_t)b * a.Tcap * K;
  const float4* sr[4];
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int i = 0; i < 4; ++i) sr[i] = reinterpret_cast<const float4*>(sb + (size_t)min(tg + i, T - 1) * K);
  for (int k4 = 0; k4 < K / 4; ++k4) {
    const float4 p = pr[k4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float4 v = sr[i][k4];
      acc[i] = fmaf(p.x, v.x, acc[i]);
      acc[i] = fmaf(p.y, v.y, acc[i]);
      acc[i] = fmaf(p.z, v.z, acc[i]);
      acc[i] = fmaf(p.w, v.w, acc[i]);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (tg + i < T) a.stat[((size_t)b * a.Tcap + tg + i) * a.n_coef + q] = acc[i];
}

// ---- deltas and the copy-out ------------------------------------------------------------------------------------
// feat_len <= 0: out (B, Tcap, 3 n), the row's own frames; otherwise (B, 3 n, feat_len), padded / chopped.
__global__ __launch_bounds__(256) void cqcc_tail(CqccArgs a) {
  if (!plan_ok(a.plan, a)) return;  // (the statics were not written either)
  const int b = blockIdx.y;
  const int n = a.n_coef;
  const int L = air_row_len(a.lengths, b, a.Lcap);
  const int T = 1 + L / a.hop;
  const int e = blockIdx.x * 256 + threadIdx.x;
  const bool padded = a.feat_len > 0;
  int q, t, f = 0;
  if (padded) {
    if (e >= n * a.feat_len) return;
    q = e / a.feat_len;
    f = e - q * a.feat_len;
    if (T >= a.feat_len) {
      const int st = (a.start != nullptr && T > a.feat_len) ? min(max(a.start[b], 0), T - a.feat_len) : 0;
      t = st + f;
    } else if (a.pad_mode == AIR_PAD_REPEAT) {
      t = f % T;
    } else {
      t = f < T ? f : -1;
    }
  } else {
    if (e >= a.Tcap * n) return;
    t = e / n;
    q = e - t * n;
    if (t >= T) return;
  }
  float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f;
  if (t >= 0) {
    const float* __restrict__ c = a.stat + (size_t)b * a.Tcap * n + q;
    auto at = [&](int u) { return c[(size_t)min(max(u, 0), T - 1) * n]; };
    auto dl = [&](int u) { return at(u + 1) - at(u - 1); };  // u inside [0, T - 1]
    v0 = at(t);
    v1 = dl(t);
    v2 = dl(min(t + 1, T - 1)) - dl(max(t - 1, 0));
  }
  if (padded) {
    float* __restrict__ o = a.out + (size_t)b * 3 * n * a.feat_len + f;
    o[(size_t)q * a.feat_len] = v0;
    o[(size_t)(n + q) * a.feat_len] = v1;
    o[(size_t)(2 * n + q) * a.feat_len] = v2;
  } else {
    float* __restrict__ o = a.out + ((size_t)b * a.Tcap + t) * 3 * n;
    o[q] = v0;
    o[n + q] = v1;
    o[2 * n + q] = v2;
  }
}

// ---- the yardstick of tools/bench_cqcc.py: the product kernel's MFMA stream with nothing around it.  Not part of the
// C-ABI of include/air_hip.h: int air_cqcc_mfma_loop(int blocks, int iters, float* out, air_stream_t stream) launches
// `blocks` workgroups of 4 waves, each wave issuing 3 * iters independent v_mfma_f32_32x32x2_f32 (4096 flop each). ----
__global__ __launch_bounds__(NT, 2) void cqcc_mfma_loop(float* out, int iters) {
  f32x16 acc[3];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[c][r] = 0.0f;
  const float a = (float)(threadIdx.x & 3), b = 1.0f + (float)(threadIdx.x & 1);
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[c], 0, 0, 0);
  }
  float sum = 0.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) sum += acc[c][r];
  if (sum == 12345.678f) out[0] = sum;  // (keeps the loop alive; never true)
}

// ---- host ---------------------------------------------------------------------------------------------------------
size_t align4(size_t n) { return (n + 3) & ~(size_t)3; }

struct WsLayout {
  size_t levels, spec, stat, total;  // floats
  long lvl_off[MAXO];
  int lvl_len[MAXO];
};

bool geometry_ok(int B, int Lcap, int O, int hop, int n_coef) {
  return B > 0 && B <= 65535 && Lcap > 0 && O >= 1 && O <= MAXO && hop >= 1 && hop <= MAXHOP && n_coef >= 1 &&
         n_coef <= MAXQ;
}

WsLayout ws_layout(int B, int Lcap, int O, int hop, int n_coef) {
  WsLayout w;
  memset(&w, 0, sizeof(w));
  size_t off = 0;
  w.lvl_len[0] = Lcap;
  for (int s = 1; s <= O - 2; ++s) {
    w.lvl_len[s] = (int)(((long)Lcap + (1L << s) - 1) >> s);
    w.lvl_off[s] = (long)off;
    off = align4(off + (size_t)B * w.lvl_len[s]);
  }
  const size_t Tcap = 1 + Lcap / hop;
  w.levels = off;
  w.spec = align4((size_t)B * Tcap * NBIN * O);
  w.stat = align4((size_t)B * Tcap * n_coef);
  w.total = w.levels + w.spec + w.stat;
  return w;
}

double bessel_i0(double x) {
  double sum = 1.0, term = 1.0;
  const double q = x * x / 4.0;
  for (int k = 1; k < 500; ++k) {
    term *= q / ((double)k * k);
    sum += term;
    if (term < 1e-18 * sum) break;
  }
  return sum;
}

// atoms of one table: ratio = R / f of bin 0 (4 for the top octave, 8 for the others); returns the half-length H
int fill_atoms(float* tab, int rows, double ratio, double Q) {
  int hl[NBIN], H = 0;
  for (int j = 0; j < NBIN; ++j) {
    hl[j] = (int)floor(Q * (ratio * exp2(-(double)j / NBIN)) / 2.0);
    if (hl[j] > H) H = hl[j];
  }
  if (2 * H + 1 > rows) return -1;
  for (int j = 0; j < NBIN; ++j) {
    const int N = 2 * hl[j] + 1;
    const double fr = exp2((double)j / NBIN) / ratio;  // f / R
    double sw = 0.0;
    for (int n = 0; n < N; ++n) sw += 0.5 - 0.5 * cos(2.0 * CQ_PI * n / (N - 1));
    for (int n = 0; n < N; ++n) {
      const double w = (0.5 - 0.5 * cos(2.0 * CQ_PI * n / (N - 1))) / sw;
      const int m = n - hl[j];
      const double ph = 2.0 * CQ_PI * fr * m;
      tab[(size_t)(H + m) * NCOL + atom_col(j, 0)] = (float)(w * cos(ph));
      tab[(size_t)(H + m) * NCOL + atom_col(j, 1)] = (float)(-w * sin(ph));
    }
  }
  return H;
}

int cqcc_run(const float* pcm, const short* pcm16, int B, int Lcap, const int* lengths, float* out, int feat_len,
             const int* start, const void* plan_dev, int O, int hop, int n_coef, int pad_mode, void* ws,
             size_t ws_bytes, bool spectrum_only, hipStream_t stream) {
  if ((pcm != nullptr) == (pcm16 != nullptr) || !out || !plan_dev || !geometry_ok(B, Lcap, O, hop, n_coef))
    return AIR_EINVAL;
  const WsLayout w = ws_layout(B, Lcap, O, hop, n_coef);
  const size_t need = (spectrum_only ? w.levels : w.total) * sizeof(float);
  if (need > 0 && (!ws || ws_bytes < need)) return AIR_EWORKSPACE;
  CqccArgs a;
  memset(&a, 0, sizeof(a));
  a.pcm = pcm;
  a.pcm16 = pcm16;
  a.plan = reinterpret_cast<const CqccPlan*>(plan_dev);
  a.lengths = lengths;
  a.start = start;
  a.levels = reinterpret_cast<float*>(ws);
  a.spec = spectrum_only ? out : a.levels + w.levels;
  a.stat = spectrum_only ? nullptr : a.levels + w.levels + w.spec;
  a.out = out;
  for (int s = 0; s < MAXO; ++s) {
    a.lvl_off[s] = w.lvl_off[s];
    a.lvl_len[s] = w.lvl_len[s];
  }
  a.B = B;
  a.Lcap = Lcap;
  a.Tcap = 1 + Lcap / hop;
  a.O = O;
  a.hop = hop;
  a.n_coef = n_coef;
  a.K = NBIN * O;
  a.feat_len = feat_len;
  a.pad_mode = pad_mode;
  for (int s = 0; s + 1 <= O - 2; ++s) {
    const dim3 grid((unsigned)((a.lvl_len[s + 1] + 255) / 256), (unsigned)B);
    hipLaunchKernelGGL(cqcc_pyramid, grid, dim3(256), 0, stream, a, s);
    AIR_CHECK_LAUNCH();
  }
  {
    const dim3 grid((unsigned)((a.Tcap + FT - 1) / FT), (unsigned)O, (unsigned)B);
    hipLaunchKernelGGL(cqcc_product, grid, dim3(NT), 0, stream, a);
    AIR_CHECK_LAUNCH();
  }
  if (spectrum_only) return AIR_OK;
  {
    const dim3 grid((unsigned)((a.Tcap + 31) / 32), (unsigned)B);
    hipLaunchKernelGGL(cqcc_project, grid, dim3(256), 0, stream, a);
    AIR_CHECK_LAUNCH();
  }
  {
    const long elems = feat_len > 0 ? (long)n_coef * feat_len : (long)a.Tcap * n_coef;
    if ((elems + 255) / 256 > 0x7fffffffL) return AIR_EINVAL;
    const dim3 grid((unsigned)((elems + 255) / 256), (unsigned)B);
    hipLaunchKernelGGL(cqcc_tail, grid, dim3(256), 0, stream, a);
    AIR_CHECK_LAUNCH();
  }
  return AIR_OK;
}

}  // namespace

extern "C" {

size_t air_cqcc_plan_bytes(void) { return sizeof(CqccPlan); }

int air_cqcc_plan_build(int bins_per_octave, int n_octaves, int hop, int n_coef, int d, double eps,
                        void* plan_host_out) {
  if (!plan_host_out || d < 1 || !(eps >= 0.0)) return AIR_EINVAL;
  if (bins_per_octave != NBIN || n_octaves < 1 || n_octaves > MAXO || hop < 1 || hop > MAXHOP || n_coef < 1 ||
      n_coef > MAXQ)
    return AIR_EUNSUPPORTED;
  CqccPlan* p = reinterpret_cast<CqccPlan*>(plan_host_out);
  memset(p, 0, sizeof(CqccPlan));
  const int O = n_octaves, K = NBIN * O;
  p->magic = CQCC_MAGIC;
  p->O = O;
  p->hop = hop;
  p->n_coef = n_coef;
  p->K = K;
  p->J = FIR_J;
  p->d = d;
  p->eps = (float)eps;

  // h: 0.5 sinc(m / 2) under a Kaiser window, unit DC gain
  {
    double h[FIR_J], sum = 0.0;
    const int half = (FIR_J - 1) / 2;
    for (int j = 0; j < FIR_J; ++j) {
      const int m = j - half;
      const double sinc = m == 0 ? 1.0 : sin(CQ_PI * m / 2.0) / (CQ_PI * m / 2.0);
      const double r = (double)m / half;
      h[j] = 0.5 * sinc * bessel_i0(FIR_BETA * sqrt(fmax(0.0, 1.0 - r * r))) / bessel_i0(FIR_BETA);
      sum += h[j];
    }
    for (int j = 0; j < FIR_J; ++j) p->h[j] = (float)(h[j] / sum);
  }

  const double Q = 1.0 / (exp2(1.0 / NBIN) - 1.0);
  p->H0 = fill_atoms(p->atoms0, KP0, 4.0, Q);
  p->H1 = fill_atoms(p->atoms1, KP1, 8.0, Q);
  if (p->H0 < 0 || p->H1 < 0) return AIR_EUNSUPPORTED;

  // P = (orthonormal DCT-II over M points) x (linear interpolation of the K bins at g_m = fmin (1 + m / d))
  const int M = 1 + (int)floor(d * (exp2((double)(K - 1) / NBIN) - 1.0));
  p->M = M;
  double* acc = new double[(size_t)n_coef * K];
  for (size_t i = 0; i < (size_t)n_coef * K; ++i) acc[i] = 0.0;
  for (int m = 0; m < M; ++m) {
    const double pos = NBIN * log2(1.0 + (double)m / d);
    int k0 = (int)floor(pos);
    if (k0 > K - 1) k0 = K - 1;
    const double fr = pos - k0;
    for (int q = 0; q < n_coef; ++q) {
      const double c = (q == 0 ? sqrt(1.0 / M) : sqrt(2.0 / M)) * cos(CQ_PI * (m + 0.5) * q / M);
      acc[(size_t)q * K + k0] += c * (1.0 - fr);
      if (k0 + 1 < K) acc[(size_t)q * K + k0 + 1] += c * fr;
    }
  }
  for (int q = 0; q < n_coef; ++q)
    for (int k = 0; k < K; ++k) p->proj[(size_t)q * K + k] = (float)acc[(size_t)q * K + k];
  delete[] acc;
  return AIR_OK;
}

int air_cqcc_n_bins(int bins_per_octave, int n_octaves) {
  return (bins_per_octave == NBIN && n_octaves >= 1 && n_octaves <= MAXO) ? NBIN * n_octaves : AIR_EUNSUPPORTED;
}

size_t air_cqcc_ws_bytes(int B, int Lcap, int n_octaves, int hop, int n_coef) {
  if (!geometry_ok(B, Lcap, n_octaves, hop, n_coef)) return 0;
  return ws_layout(B, Lcap, n_octaves, hop, n_coef).total * sizeof(float);
}

int air_cqcc_fwd(const float* pcm, const int16_t* pcm16, int B, int L, float* out, const void* plan_dev,
                 int n_octaves, int hop, int n_coef, void* ws, size_t ws_bytes, air_stream_t stream) {
  return cqcc_run(pcm, reinterpret_cast<const short*>(pcm16), B, L, nullptr, out, 0, nullptr, plan_dev, n_octaves, hop,
                  n_coef, AIR_PAD_REPEAT, ws, ws_bytes, false, air_stream(stream));
}

int air_cqcc_fwd_ragged(const float* pcm, const int16_t* pcm16, int B, int Lcap, const int* lengths_dev, float* out,
                        int feat_len, const int* start_dev, const void* plan_dev, int n_octaves, int hop, int n_coef,
                        int pad_mode, void* ws, size_t ws_bytes, air_stream_t stream) {
  if (pad_mode == AIR_PAD_SILENCE) return AIR_EUNSUPPORTED;  // the silence frame is an LFCC frame (dataset.py:13-16)
  if (pad_mode != AIR_PAD_REPEAT && pad_mode != AIR_PAD_ZERO) return AIR_EINVAL;
  return cqcc_run(pcm, reinterpret_cast<const short*>(pcm16), B, Lcap, lengths_dev, out, feat_len, start_dev, plan_dev,
                  n_octaves, hop, n_coef, pad_mode, ws, ws_bytes, false, air_stream(stream));
}

int air_cqcc_spectrum(const float* pcm, const int16_t* pcm16, int B, int Lcap, const int* lengths_dev, float* out,
                      const void* plan_dev, int n_octaves, int hop, int n_coef, void* ws, size_t ws_bytes,
                      air_stream_t stream) {
  return cqcc_run(pcm, reinterpret_cast<const short*>(pcm16), B, Lcap, lengths_dev, out, 0, nullptr, plan_dev,
                  n_octaves, hop, n_coef, AIR_PAD_REPEAT, ws, ws_bytes, true, air_stream(stream));
}

int air_cqcc_mfma_loop(int blocks, int iters, float* out, air_stream_t stream);  // (bench-only: declared here)
int air_cqcc_mfma_loop(int blocks, int iters, float* out, air_stream_t stream) {
  if (blocks <= 0 || iters <= 0 || !out) return AIR_EINVAL;
  hipLaunchKernelGGL(cqcc_mfma_loop, dim3((unsigned)blocks), dim3(NT), 0, air_stream(stream), out, iters);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

}  // extern "C"
