// WAV payloads / ragged PCM of any served rate -> a ragged (B, Lcap_out) batch at the target rate, in one launch
// (raw_dataset.py:20-28: librosa.load(sr=16000) of a .wav).  Sample-format conversion, down-mix and the band-limited
// sinc interpolation of include/air_hip.h ("Resample") are fused: a row never exists at its source rate on the device.
//
//   host   air_resample_geometry / air_resample_table_host: (L, M, K) of a rate pair and its L x K coefficient table,
//          evaluated in fp64 (Kaiser window, I0 by its power series) and rounded once to fp32.  No HIP call.
//   device resample_kernel<RAGGED>: one workgroup per (row, tile of `tile` outputs).  The tile's input window
//          [floor(t0 M / L) - H + 1, floor(t1 M / L) + H] is fetched, converted and down-mixed ONCE into LDS as fp32
//          (zeros outside [0, n)); lanes take consecutive outputs, each an ascending-j fmaf chain over its K taps in four
//          interleaved accumulators (j mod 4), summed (a0 + a1) + (a2 + a3).  The coefficient table of the row's rate
//          is copied into LDS when it fits (kTableLds floats: 8 / 24 / 32 / 48 kHz -> 16 kHz), read through L2
//          otherwise (44.1 kHz: 160 x 354).  L == M is the identity path: fetch, convert, store - no table, no sum.
//          float and int16 outputs share the accumulation; int16 = saturating round-half-even of 32768 y.
//
// Bounds: a row's bytes are [start, end) = [(byte_off[b] + 3) & ~3, byte_off[b + 1]) clipped to total_bytes (RAGGED:
// row b of the dense batch); frames * block_align must fit in it and ceil(frames L / M) in Lcap_out, or the row is
// zeros with status AIR_WAV_LENGTH_MISMATCH; an unknown format code or rate index: AIR_WAV_BAD_FORMAT.  Every fetch
// is of a frame index inside [0, frames); every store is at t < Lcap_out of the row.  The window holds at most
// tile * M / L + K + 2 samples, which the host sizes `tile` for (kWindow floats).
#include <math.h>

#include "air_common.h"
#include "air_options.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWindow = 8192;    // fp32 samples of the input window in LDS
constexpr int kTableLds = 4096;  // fp32 coefficients in LDS beside it
constexpr double kZ = 64.0, kR = 0.9475937167399596, kBeta = 14.769656459379492;

struct Args {
  const uint8_t* bytes;   // wav: the packed payloads; ragged: the dense batch
  size_t total_bytes;
  const int* byte_off;    // wav only
  const int* frames;      // wav: frames of row b; ragged: samples of row b
  const int* fmt;         // wav only
  const int* rate_idx;
  const float* tables;
  int16_t* y16;
  float* y32;
  int* status;
  int Lcap_in;            // ragged only
  int in_fmt;             // ragged only: the format code of every row
  int Lcap_out;
  int tile;
  int table_lds;
  air_resample_desc desc;
};

int64_t gcd64(int64_t a, int64_t b) {
  while (b) {
    const int64_t t = a % b;
    a = b;
    b = t;
  }
  return a;
}

double bessel_i0(double x) {  // sum_k ((x / 2)^k / k!)^2
  const double q = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 500; ++k) {
    term *= q / ((double)k * (double)k);
    sum += term;
    if (term < 1e-18 * sum) break;
  }
  return sum;
}

double sinc_pi(double x) {
  const double kPi = 3.14159265358979323846;
  if (x == 0.0) return 1.0;
  return sin(kPi * x) / (kPi * x);
}

int bytes_of_kind(int kind) {
  switch (kind) {
    case AIR_PCM_U8: return 1;
    case AIR_PCM_S16: return 2;
    case AIR_PCM_S24: return 3;
    case AIR_PCM_S32: return 4;
    case AIR_PCM_F32: return 4;
    case AIR_PCM_F64: return 8;
  }
  return 0;
}

bool desc_ok(const air_resample_desc* d, const float* tables, size_t table_elems) {
  if (!d || d->nrates < 1 || d->nrates > AIR_RESAMPLE_MAX_RATES) return false;
  for (int r = 0; r < d->nrates; ++r) {
    const air_resample_rate& q = d->rate[r];
    if (q.L < 1 || q.L > AIR_RESAMPLE_MAX_L || q.M < 1 || q.K < 0 || q.K > AIR_RESAMPLE_MAX_K || (q.K & 1)) return false;
    if (q.L == q.M) {
      if (q.L != 1 || q.K != 0) return false;
      continue;
    }
    if (q.K < 2 || q.table_off < 0 || !tables) return false;
    if ((size_t)q.table_off + (size_t)q.L * q.K > table_elems) return false;
    // the window of the smallest tile has to fit: 64 * M / L + K + 2
    if (((int64_t)64 * q.M) / q.L + q.K + 2 > kWindow) return false;
  }
  return true;
}

int pick_tile(const air_resample_desc* d) {
  int tile = 1024;
  for (int r = 0; r < d->nrates; ++r) {
    const air_resample_rate& q = d->rate[r];
    if (q.L == q.M) continue;
    while (tile > 64 && ((int64_t)tile * q.M) / q.L + q.K + 2 > kWindow) tile >>= 1;
  }
  return tile;
}

__device__ __forceinline__ float sample_at(const uint8_t* p, int kind) {
  switch (kind) {
    case AIR_PCM_U8: return ((float)p[0] - 128.0f) * (1.0f / 128.0f);
    case AIR_PCM_S16: return (float)*reinterpret_cast<const int16_t*>(p) * (1.0f / 32768.0f);
    case AIR_PCM_S24: {
      const int v = (int)((uint32_t)p[0] << 8 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 24) >> 8;
      return (float)v * (1.0f / 8388608.0f);
    }
    case AIR_PCM_S32: return (float)*reinterpret_cast<const int32_t*>(p) * (1.0f / 2147483648.0f);
    case AIR_PCM_F32: return *reinterpret_cast<const float*>(p);
    default: {  // AIR_PCM_F64: rows start 4-byte aligned, not 8
      const uint32_t lo = *reinterpret_cast<const uint32_t*>(p), hi = *reinterpret_cast<const uint32_t*>(p + 4);
      return (float)__longlong_as_double((long long)((unsigned long long)hi << 32 | lo));
    }
  }
}

// frame i of a row (0 <= i < frames, checked by the caller): converted, summed over the channels in order, / C
__device__ __forceinline__ float frame_at(const uint8_t* row, int64_t i, int kind, int bps, int C) {
  const uint8_t* p = row + (size_t)i * (size_t)(bps * C);
  if (C == 1) return sample_at(p, kind);
  float s = sample_at(p, kind);
  for (int c = 1; c < C; ++c) s = s + sample_at(p + c * bps, kind);
  return s / (float)C;
}

__device__ __forceinline__ void store_out(const Args& a, size_t at, float v) {
  if (a.y32) a.y32[at] = v;
  if (a.y16) {
    float q = rintf(v * 32768.0f);  // round half to even
    q = q > 32767.0f ? 32767.0f : (q < -32768.0f ? -32768.0f : q);
    a.y16[at] = (int16_t)(v != v ? 0 : (int)q);
  }
}

template <typename Table>
__device__ __forceinline__ float taps(Table c, const float* w, int K) {
  float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
  int j = 0;
  for (; j + 4 <= K; j += 4) {
    a0 = fmaf(c[j], w[j], a0);
    a1 = fmaf(c[j + 1], w[j + 1], a1);
    a2 = fmaf(c[j + 2], w[j + 2], a2);
    a3 = fmaf(c[j + 3], w[j + 3], a3);
  }
  if (j < K) a0 = fmaf(c[j], w[j], a0);  // K is even: two taps are left at most
  if (j + 1 < K) a1 = fmaf(c[j + 1], w[j + 1], a1);
  return (a0 + a1) + (a2 + a3);
}

template <bool RAGGED>
__global__ __launch_bounds__(kThreads) void resample_kernel(const Args a) {
  __shared__ float win[kWindow];
  __shared__ float tab[kTableLds];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int Lcap = a.Lcap_out;
  const int64_t t0 = (int64_t)blockIdx.x * a.tile;
  if (t0 >= Lcap) return;
  const int64_t tcap = t0 + a.tile < Lcap ? t0 + a.tile : Lcap;  // this workgroup stores [t0, tcap) of row b
  const size_t out = (size_t)b * (size_t)Lcap;

  // ---- the row: every value below is the same in all lanes
  int status = AIR_WAV_OK;
  const int code = RAGGED ? a.in_fmt : a.fmt[b];
  const int kind = code & 15, bps = (code >> 4) & 15, C = (code >> 8) & 255;
  const int ridx = a.rate_idx[b];
  int64_t n = a.frames[b];
  size_t start, end;
  if (RAGGED) {
    start = (size_t)b * (size_t)a.Lcap_in * (size_t)bps;
    end = start + (size_t)a.Lcap_in * (size_t)bps;
  } else {
    const int o0 = a.byte_off[b], o1 = a.byte_off[b + 1];
    start = o0 < 0 ? 0 : ((size_t)o0 + 3) & ~(size_t)3;
    end = o1 < 0 ? 0 : (size_t)o1;
  }
  if (end > a.total_bytes) end = a.total_bytes;
  bool fmt_ok = (code >> 16) == 0 && C >= 1 && C <= AIR_WAV_MAX_CHANNELS && kind <= AIR_PCM_F64;
  if (fmt_ok) {
    const int want = kind == AIR_PCM_U8 ? 1 : kind == AIR_PCM_S16 ? 2 : kind == AIR_PCM_S24 ? 3 : kind == AIR_PCM_F64 ? 8 : 4;
    fmt_ok = bps == want;
  }
  int L = 1, M = 1, K = 0, toff = 0;
  if (!fmt_ok || ridx < 0 || ridx >= a.desc.nrates) {
    status = AIR_WAV_BAD_FORMAT;
  } else {
    L = a.desc.rate[ridx].L;
    M = a.desc.rate[ridx].M;
    K = a.desc.rate[ridx].K;
    toff = a.desc.rate[ridx].table_off;
  }
  int64_t n_out = 0;
  if (status == AIR_WAV_OK) {
    if (n < 0 || start > end || (uint64_t)n * (uint64_t)(bps * C) > (uint64_t)(end - start)) {
      status = AIR_WAV_LENGTH_MISMATCH;
    } else {
      n_out = (n * L + M - 1) / M;
      if (n_out > Lcap) status = AIR_WAV_LENGTH_MISMATCH;
    }
  }
  if (blockIdx.x == 0 && tid == 0) a.status[b] = status;
  if (status != AIR_WAV_OK) n_out = 0;
  const int64_t t1 = tcap < n_out ? tcap : n_out;  // outputs [t0, t1) carry signal, [t1, tcap) are zero
  for (int64_t t = (t0 > t1 ? t0 : t1) + tid; t < tcap; t += kThreads) store_out(a, out + (size_t)t, 0.0f);
  if (t1 <= t0) return;
  const uint8_t* row = a.bytes + start;

  if (L == M) {  // identity: format conversion and down-mix only
    for (int64_t t = t0 + tid; t < t1; t += kThreads) store_out(a, out + (size_t)t, frame_at(row, t, kind, bps, C));
    return;
  }

  // ---- the window [first, last] of input samples of outputs [t0, t1)
  const int H = K >> 1;
  const int64_t first = (t0 * M) / L - H + 1, last = ((t1 - 1) * M) / L + H;
  const int W = (int)(last - first + 1);  // <= tile * M / L + K + 1 <= kWindow (host: pick_tile)
  if (W > kWindow) return;                // (cannot happen; nothing is read beyond the window)
  if (kind == AIR_PCM_S16 && C == 1 && ((uintptr_t)row & 3) == 0) {
    // the corpora's case: aligned 4-byte loads of sample pairs (a packed row starts 4-byte aligned)
    const int64_t even = first & ~(int64_t)1;  // floor to even, also for negative `first`
    for (int q = tid; 2 * q <= W; q += kThreads) {
      const int64_t i = even + 2 * (int64_t)q;
      float v0 = 0.0f, v1 = 0.0f;
      if (i >= 0 && i + 1 < n) {
        const uint32_t u = *reinterpret_cast<const uint32_t*>(row + (size_t)i * 2);
        v0 = (float)(int16_t)(u & 0xffffu) * (1.0f / 32768.0f);
        v1 = (float)(int16_t)(u >> 16) * (1.0f / 32768.0f);
      } else {
        if (i >= 0 && i < n) v0 = sample_at(row + (size_t)i * 2, AIR_PCM_S16);
        if (i + 1 >= 0 && i + 1 < n) v1 = sample_at(row + (size_t)(i + 1) * 2, AIR_PCM_S16);
      }
      const int64_t w0 = i - first;
      if (w0 >= 0 && w0 < W) win[w0] = v0;
      if (w0 + 1 >= 0 && w0 + 1 < W) win[w0 + 1] = v1;
    }
  } else {
    for (int q = tid; q < W; q += kThreads) {
      const int64_t i = first + q;
      win[q] = (i >= 0 && i < n) ? frame_at(row, i, kind, bps, C) : 0.0f;
    }
  }
  const float* table = a.tables + toff;
  const bool in_lds = a.table_lds && L * K <= kTableLds;
  if (in_lds)
    for (int q = tid; q < L * K; q += kThreads) tab[q] = table[q];
  __syncthreads();

  for (int64_t t = t0 + tid; t < t1; t += kThreads) {
    const int64_t tm = t * M;
    const int64_t n0 = tm / L;
    const int p = (int)(tm - n0 * L);
    const float* w = win + (int)(n0 - H + 1 - first);  // [0, W - K]: n0 >= floor(t0 M / L), n0 + H <= last
    const float y = in_lds ? taps(tab + p * K, w, K) : taps(table + (size_t)p * K, w, K);
    store_out(a, out + (size_t)t, y);
  }
}

int launch(bool ragged, Args& a, int B, air_stream_t stream) {
  a.tile = pick_tile(&a.desc);
  a.table_lds = air_opt(AIR_OPT_RESAMPLE_TABLE_LDS) != 0;
  const dim3 grid((unsigned)((a.Lcap_out + a.tile - 1) / a.tile), (unsigned)B);
  hipStream_t st = air_stream(stream);
  if (ragged)
    hipLaunchKernelGGL(resample_kernel<true>, grid, dim3(kThreads), 0, st, a);
  else
    hipLaunchKernelGGL(resample_kernel<false>, grid, dim3(kThreads), 0, st, a);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

}  // namespace

extern "C" {

int air_resample_geometry(int sr_in, int sr_out, int* L, int* M, int* K) {
  if (sr_in < 1 || sr_out < 1 || !L || !M || !K) return AIR_EINVAL;
  const int64_t g = gcd64(sr_in, sr_out);
  const int64_t l = sr_out / g, m = sr_in / g;
  if (l > AIR_RESAMPLE_MAX_L) return AIR_EINVAL;
  int k = 0;
  if (l != m) {
    // H = ceil(Z / s), s = min(1, L / M): Z exactly when upsampling, ceil(Z M / L) in integers otherwise
    const int64_t h = l >= m ? (int64_t)kZ : ((int64_t)kZ * m + l - 1) / l;
    if (2 * h > AIR_RESAMPLE_MAX_K) return AIR_EINVAL;
    k = (int)(2 * h);
  }
  *L = (int)l;
  *M = (int)m;
  *K = k;
  return AIR_OK;
}

int air_resample_table_host(int sr_in, int sr_out, float* table) {
  int L, M, K;
  if (!table) return AIR_EINVAL;
  const int rc = air_resample_geometry(sr_in, sr_out, &L, &M, &K);
  if (rc != AIR_OK) return rc;
  const int H = K / 2;
  const double s = L < M ? (double)L / (double)M : 1.0;
  const double i0b = bessel_i0(kBeta);
  for (int p = 0; p < L; ++p)
    for (int j = 0; j < K; ++j) {
      const double u = s * ((double)p / (double)L + (double)(H - 1 - j));
      double h = 0.0;
      if (fabs(u) < kZ) {
        const double r = u / kZ;
        h = kR * sinc_pi(kR * u) * bessel_i0(kBeta * sqrt(1.0 - r * r)) / i0b;
      }
      table[(size_t)p * K + j] = (float)(s * h);
    }
  return AIR_OK;
}

int air_resample_ragged(const void* x, int in_kind, int B, int Lcap_in, const int* lengths, const int* rate_idx,
                        const air_resample_desc* desc, const float* tables, size_t table_elems, int16_t* y16, float* y32,
                        int Lcap_out, int* status, air_stream_t stream) {
  if (B < 1 || Lcap_in < 1 || Lcap_out < 1 || !x || !lengths || !rate_idx || !status || (!y16 && !y32)) return AIR_EINVAL;
  if (in_kind != AIR_PCM_S16 && in_kind != AIR_PCM_F32) return AIR_EINVAL;
  if (!desc_ok(desc, tables, table_elems)) return AIR_EINVAL;
  if ((const void*)y16 == x || (const void*)y32 == x || ((uintptr_t)x & 3)) return AIR_EINVAL;
  if ((int64_t)B * Lcap_in > ((int64_t)1 << 40) || (int64_t)B * Lcap_out > ((int64_t)1 << 40)) return AIR_EINVAL;
  if (B > 65535) return AIR_EUNSUPPORTED;
  Args a = {};
  const int bps = bytes_of_kind(in_kind);
  a.bytes = static_cast<const uint8_t*>(x);
  a.total_bytes = (size_t)B * (size_t)Lcap_in * (size_t)bps;
  a.frames = lengths;
  a.rate_idx = rate_idx;
  a.tables = tables;
  a.y16 = y16;
  a.y32 = y32;
  a.status = status;
  a.Lcap_in = Lcap_in;
  a.in_fmt = AIR_WAV_FMT(in_kind, bps, 1);
  a.Lcap_out = Lcap_out;
  a.desc = *desc;
  return launch(true, a, B, stream);
}

int air_wav_decode(const uint8_t* bytes, size_t total_bytes, const int* byte_off, const int* frames, const int* fmt,
                   const int* rate_idx, int B, const air_resample_desc* desc, const float* tables, size_t table_elems,
                   int16_t* y16, float* y32, int Lcap_out, int* status, air_stream_t stream) {
  if (B < 1 || Lcap_out < 1 || total_bytes < 1 || total_bytes > (size_t)0x7fffffff) return AIR_EINVAL;
  if (!bytes || !byte_off || !frames || !fmt || !rate_idx || !status || (!y16 && !y32)) return AIR_EINVAL;
  if (!desc_ok(desc, tables, table_elems)) return AIR_EINVAL;
  if ((uintptr_t)bytes & 3) return AIR_EINVAL;
  if ((int64_t)B * Lcap_out > ((int64_t)1 << 40)) return AIR_EINVAL;
  if (B > 65535) return AIR_EUNSUPPORTED;
  Args a = {};
  a.bytes = bytes;
  a.total_bytes = total_bytes;
  a.byte_off = byte_off;
  a.frames = frames;
  a.fmt = fmt;
  a.rate_idx = rate_idx;
  a.tables = tables;
  a.y16 = y16;
  a.y32 = y32;
  a.status = status;
  a.Lcap_out = Lcap_out;
  a.desc = *desc;
  return launch(false, a, B, stream);
}

}  // extern "C"
