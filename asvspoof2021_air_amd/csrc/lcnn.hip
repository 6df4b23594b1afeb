// LCNN (model.py:511-610, the reference's default --model): the kernels its layers need beyond the generic
// convolutions, BatchNorm and linear kernels.
//   * conv1 fused: 5x5 / Cin 1 / 64-output convolution + bias + Max-Feature-Map + 2x2 max-pool in one pass; the
//     64 x H x W pre-MFM map (11.5 MB per 4 s utterance) never reaches HBM.  Its weight / bias gradient reads the
//     pooled gradient and the route bytes.
//   * MFM (+ optional 2x2 floor-mode max-pool) forward over a generic conv's output, with the bias added on the
//     way in, and its route backward + bias gradient.
// Route byte of every post-MFM / post-pool element: bits 0-1 the winning window position (dy * 2 + dx, 0 without
// pooling), bit 2 the MFM half (0: channel c, 1: channel c + C/2).  Ties go to the first candidate (half 0; the
// first window position in row-major order), as torch's max / max_pool2d do.
#include <cstdint>

#include "air_common.h"

namespace {

constexpr int NT = 256;
constexpr int C1_CO = 64;       // conv1 output channels (before MFM)
constexpr int C1_TAPS = 25;     // 5 x 5
constexpr int WG_CHUNKS = 128;  // position chunks of the conv1 weight gradient (partials reduced in index order)
constexpr int BG_CHUNKS = 16;   // position chunks of the MFM bias gradient

inline unsigned nblk(size_t n) { return (unsigned)((n + NT - 1) / NT); }

// ---------------------------------------------------------------------------------------------- conv1 forward
// One thread per pooled output pixel (b, ho, wo), all 32 channel pairs: the 6 x 6 input patch under the 2 x 2
// window of 5 x 5 taps lives in registers, the weights in LDS (wave-uniform broadcast reads).
__global__ __launch_bounds__(NT) void conv1_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                       const float* __restrict__ bias, int B, int H, int W, int Hp,
                                                       int Wp, float* __restrict__ y, uint8_t* __restrict__ route) {
  __shared__ float sw[C1_CO * C1_TAPS];
  __shared__ float sb[C1_CO];
  for (int i = threadIdx.x; i < C1_CO * C1_TAPS; i += NT) sw[i] = w[i];
  for (int i = threadIdx.x; i < C1_CO; i += NT) sb[i] = bias[i];
  __syncthreads();
  const size_t npix = (size_t)B * Hp * Wp;
  const size_t id = (size_t)blockIdx.x * NT + threadIdx.x;
  if (id >= npix) return;
  const int wo = (int)(id % Wp);
  const int ho = (int)((id / Wp) % Hp);
  const int b = (int)(id / ((size_t)Wp * Hp));
  const float* xb = x + (size_t)b * H * W;
  float p[6][6];
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    const int hi = 2 * ho + r - 2;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      const int wi = 2 * wo + c - 2;
      p[r][c] = (hi >= 0 && hi < H && wi >= 0 && wi < W) ? xb[(size_t)hi * W + wi] : 0.0f;
    }
  }
  const int C2 = C1_CO / 2;
  const size_t plane = (size_t)Hp * Wp;
  const size_t obase = (size_t)b * C2 * plane + (size_t)ho * Wp + wo;
  for (int c = 0; c < C2; ++c) {
    float best = 0.0f;
    int br = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int dy = q >> 1, dx = q & 1;
      float a0 = 0.0f, a1 = 0.0f;
#pragma unroll
      for (int kh = 0; kh < 5; ++kh)
#pragma unroll
        for (int kw = 0; kw < 5; ++kw) {
          const float v = p[dy + kh][dx + kw];
          a0 = fmaf(v, sw[c * C1_TAPS + kh * 5 + kw], a0);
          a1 = fmaf(v, sw[(c + C2) * C1_TAPS + kh * 5 + kw], a1);
        }
      a0 += sb[c];
      a1 += sb[c + C2];
      const bool h1 = a1 > a0;
      const float m = h1 ? a1 : a0;
      if (q == 0 || m > best) {
        best = m;
        br = q | (h1 ? 4 : 0);
      }
    }
    y[obase + (size_t)c * plane] = best;
    route[obase + (size_t)c * plane] = (uint8_t)br;
  }
}

// ------------------------------------------------------------------------------------- conv1 weight gradient
// Block (c, chunk): the pooled positions [chunk range) of channel pair c.  Each thread keeps both halves' 25 tap
// sums + the bias sum; the block folds them in a fixed order (wave shuffles, then the 4 waves in LDS) into
// partial[chunk][c][2][26].  A second kernel sums the chunks in index order: the same bits on every run.
__global__ __launch_bounds__(NT) void conv1_wgrad_partial_kernel(const float* __restrict__ x,
                                                                 const float* __restrict__ dy,
                                                                 const uint8_t* __restrict__ route, int B, int H,
                                                                 int W, int Hp, int Wp, float* __restrict__ partial) {
  const int c = blockIdx.x, chunk = blockIdx.y;
  const int C2 = C1_CO / 2;
  const size_t plane = (size_t)Hp * Wp;
  const size_t npos = (size_t)B * plane;
  const size_t per = (npos + WG_CHUNKS - 1) / WG_CHUNKS;
  const size_t lo = per * chunk;
  const size_t hi = lo + per < npos ? lo + per : npos;
  float acc0[C1_TAPS + 1], acc1[C1_TAPS + 1];
#pragma unroll
  for (int k = 0; k <= C1_TAPS; ++k) acc0[k] = acc1[k] = 0.0f;
  for (size_t i = lo + threadIdx.x; i < hi; i += NT) {
    const int b = (int)(i / plane);
    const size_t s = i - (size_t)b * plane;
    const int ho = (int)(s / Wp), wo = (int)(s % Wp);
    const size_t o = ((size_t)b * C2 + c) * plane + s;
    const float g = dy[o];
    const int r = route[o];
    const float g0 = (r & 4) ? 0.0f : g, g1 = (r & 4) ? g : 0.0f;
    const int h0 = 2 * ho + ((r >> 1) & 1) - 2, w0 = 2 * wo + (r & 1) - 2;
    const float* xb = x + (size_t)b * H * W;
#pragma unroll
    for (int kh = 0; kh < 5; ++kh)
#pragma unroll
      for (int kw = 0; kw < 5; ++kw) {
        const int hh = h0 + kh, ww = w0 + kw;
        const float v = (hh >= 0 && hh < H && ww >= 0 && ww < W) ? xb[(size_t)hh * W + ww] : 0.0f;
        acc0[kh * 5 + kw] = fmaf(g0, v, acc0[kh * 5 + kw]);
        acc1[kh * 5 + kw] = fmaf(g1, v, acc1[kh * 5 + kw]);
      }
    acc0[C1_TAPS] += g0;
    acc1[C1_TAPS] += g1;
  }
  __shared__ float red[NT / AIR_WAVE][2 * (C1_TAPS + 1)];
  const int wave = threadIdx.x / AIR_WAVE, lane = threadIdx.x % AIR_WAVE;
#pragma unroll
  for (int k = 0; k <= C1_TAPS; ++k) {
    const float s0 = air_wave_sum(acc0[k]);
    const float s1 = air_wave_sum(acc1[k]);
    if (lane == 0) {
      red[wave][k] = s0;
      red[wave][C1_TAPS + 1 + k] = s1;
    }
  }
  __syncthreads();
  if (threadIdx.x < 2 * (C1_TAPS + 1)) {
    float s = 0.0f;
    for (int wv = 0; wv < NT / AIR_WAVE; ++wv) s += red[wv][threadIdx.x];
    partial[((size_t)chunk * C2 + c) * 2 * (C1_TAPS + 1) + threadIdx.x] = s;
  }
}

// dw[co][k], db[co] = sum over chunks of partial[chunk][co % 32][co / 32][k] (k = 25: the bias)
__global__ __launch_bounds__(NT) void conv1_wgrad_final_kernel(const float* __restrict__ partial,
                                                               float* __restrict__ dw, float* __restrict__ db) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= C1_CO * (C1_TAPS + 1)) return;
  const int co = i / (C1_TAPS + 1), k = i % (C1_TAPS + 1);
  const int C2 = C1_CO / 2;
  const int c = co % C2, h = co / C2;
  float s = 0.0f;
  for (int ch = 0; ch < WG_CHUNKS; ++ch) s += partial[((size_t)ch * C2 + c) * 2 * (C1_TAPS + 1) + h * (C1_TAPS + 1) + k];
  if (k < C1_TAPS)
    dw[co * C1_TAPS + k] = s;
  else
    db[co] = s;
}

// --------------------------------------------------------------------------------------------- MFM (+ pool)
// x: (B, Ctot, H, W), channels [0, C) used (C <= Ctot: a conv run with zero-padded weight rows); y, route:
// (B, C/2, Ho, Wo) with Ho = H / 2, Wo = W / 2 when pooling (floor), else H, W.
__global__ __launch_bounds__(NT) void mfm_pool_fwd_kernel(const float* __restrict__ x, const float* __restrict__ bias,
                                                          int B, int Ctot, int C, int H, int W, int pool, int Ho,
                                                          int Wo, float* __restrict__ y, uint8_t* __restrict__ route) {
  const int C2 = C / 2;
  const size_t n = (size_t)B * C2 * Ho * Wo;
  const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  const int wo = (int)(i % Wo);
  const int ho = (int)((i / Wo) % Ho);
  const int c = (int)((i / ((size_t)Wo * Ho)) % C2);
  const int b = (int)(i / ((size_t)Wo * Ho * C2));
  const size_t plane = (size_t)H * W;
  const float* x0 = x + ((size_t)b * Ctot + c) * plane;
  const float* x1 = x0 + (size_t)C2 * plane;
  const float b0 = bias ? bias[c] : 0.0f, b1 = bias ? bias[c + C2] : 0.0f;
  const int nq = pool ? 4 : 1;
  float best = 0.0f;
  int br = 0;
  for (int q = 0; q < nq; ++q) {
    const int hh = pool ? 2 * ho + (q >> 1) : ho, ww = pool ? 2 * wo + (q & 1) : wo;
    const size_t s = (size_t)hh * W + ww;
    const float a0 = bias ? x0[s] + b0 : x0[s];
    const float a1 = bias ? x1[s] + b1 : x1[s];
    const bool h1 = a1 > a0;
    const float m = h1 ? a1 : a0;
    if (q == 0 || m > best) {
      best = m;
      br = q | (h1 ? 4 : 0);
    }
  }
  y[i] = best;
  route[i] = (uint8_t)br;
}

// dx (B, Ctot, H, W), every element written: dy where the element won its MFM pair and pool window, else 0
// (losers, the row / column floor-mode pooling dropped, the padded channels [C, Ctot))
__global__ __launch_bounds__(NT) void mfm_pool_bwd_kernel(const float* __restrict__ dy,
                                                          const uint8_t* __restrict__ route, int B, int Ctot, int C,
                                                          int H, int W, int pool, int Ho, int Wo,
                                                          float* __restrict__ dx) {
  const size_t n = (size_t)B * Ctot * H * W;
  const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  const int w = (int)(i % W);
  const int h = (int)((i / W) % H);
  const int ch = (int)((i / ((size_t)W * H)) % Ctot);
  const int b = (int)(i / ((size_t)W * H * Ctot));
  const int C2 = C / 2;
  float v = 0.0f;
  if (ch < C) {
    const int c = ch < C2 ? ch : ch - C2, half = ch < C2 ? 0 : 4;
    const int ho = pool ? h >> 1 : h, wo = pool ? w >> 1 : w;
    if (ho < Ho && wo < Wo) {
      const size_t o = (((size_t)b * C2 + c) * Ho + ho) * Wo + wo;
      const int q = pool ? ((h & 1) << 1) | (w & 1) : 0;
      if (route[o] == (uint8_t)(q | half)) v = dy[o];
    }
  }
  dx[i] = v;
}

// Bias gradient = channel sums of the pre-MFM gradient = sums of dy over the positions each half won.
// Block (c, chunk) -> partial[c][chunk][2]; the final kernel folds the chunks in index order.
__global__ __launch_bounds__(NT) void mfm_bias_partial_kernel(const float* __restrict__ dy,
                                                              const uint8_t* __restrict__ route, int B, int C2,
                                                              int S, float* __restrict__ partial) {
  const int c = blockIdx.x, chunk = blockIdx.y;
  const size_t npos = (size_t)B * S;
  const size_t per = (npos + BG_CHUNKS - 1) / BG_CHUNKS;
  const size_t lo = per * chunk;
  const size_t hi = lo + per < npos ? lo + per : npos;
  float s0 = 0.0f, s1 = 0.0f;
  for (size_t i = lo + threadIdx.x; i < hi; i += NT) {
    const int b = (int)(i / S);
    const size_t o = ((size_t)b * C2 + c) * S + (i - (size_t)b * S);
    const float g = dy[o];
    if (route[o] & 4)
      s1 += g;
    else
      s0 += g;
  }
  __shared__ float red[NT / AIR_WAVE][2];
  const int wave = threadIdx.x / AIR_WAVE, lane = threadIdx.x % AIR_WAVE;
  s0 = air_wave_sum(s0);
  s1 = air_wave_sum(s1);
  if (lane == 0) {
    red[wave][0] = s0;
    red[wave][1] = s1;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    float s = 0.0f;
    for (int wv = 0; wv < NT / AIR_WAVE; ++wv) s += red[wv][threadIdx.x];
    partial[((size_t)c * BG_CHUNKS + chunk) * 2 + threadIdx.x] = s;
  }
}

__global__ __launch_bounds__(NT) void mfm_bias_final_kernel(const float* __restrict__ partial, int C2,
                                                            float* __restrict__ db) {
  const int ch = blockIdx.x * NT + threadIdx.x;
  if (ch >= 2 * C2) return;
  const int c = ch < C2 ? ch : ch - C2, h = ch < C2 ? 0 : 1;
  float s = 0.0f;
  for (int k = 0; k < BG_CHUNKS; ++k) s += partial[((size_t)c * BG_CHUNKS + k) * 2 + h];
  db[ch] = s;
}

// ------------------------------------------------------------------------------------------------- helpers
// dst[i] = src[i] for i < min(n_dst, n_src), 0 for n_src <= i < n_dst
__global__ __launch_bounds__(NT) void copy_pad_kernel(float* __restrict__ dst, size_t n_dst,
                                                      const float* __restrict__ src, size_t n_src) {
  const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n_dst) return;
  dst[i] = i < n_src ? src[i] : 0.0f;
}

__global__ __launch_bounds__(NT) void mul_kernel(const float* __restrict__ a, const float* __restrict__ b, size_t n,
                                                 float* __restrict__ y) {
  const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
  if (i < n) y[i] = a[i] * b[i];
}

}  // namespace

extern "C" {

size_t air_lcnn_conv1_wgrad_ws_bytes(void) {
  return (size_t)WG_CHUNKS * (C1_CO / 2) * 2 * (C1_TAPS + 1) * sizeof(float);
}

size_t air_mfm_bias_grad_ws_bytes(int C) {
  if (C <= 0 || C % 2) return 0;
  return (size_t)(C / 2) * BG_CHUNKS * 2 * sizeof(float);
}

int air_lcnn_conv1_fwd(const float* x, const float* w, const float* bias, int B, int H, int W, float* y,
                       uint8_t* route, air_stream_t stream) {
  if (!x || !w || !bias || !y || !route || B <= 0 || H < 2 || W < 2) return AIR_EINVAL;
  const int Hp = H / 2, Wp = W / 2;
  hipLaunchKernelGGL(conv1_fwd_kernel, dim3(nblk((size_t)B * Hp * Wp)), dim3(NT), 0, air_stream(stream), x, w, bias,
                     B, H, W, Hp, Wp, y, route);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

int air_lcnn_conv1_wgrad(const float* x, const float* dy, const uint8_t* route, int B, int H, int W, float* dw,
                         float* db, void* ws, size_t ws_bytes, air_stream_t stream) {
  if (!x || !dy || !route || !dw || !db || !ws || B <= 0 || H < 2 || W < 2) return AIR_EINVAL;
  if (ws_bytes < air_lcnn_conv1_wgrad_ws_bytes()) return AIR_EWORKSPACE;
  float* partial = static_cast<float*>(ws);
  hipLaunchKernelGGL(conv1_wgrad_partial_kernel, dim3(C1_CO / 2, WG_CHUNKS), dim3(NT), 0, air_stream(stream), x, dy,
                     route, B, H, W, H / 2, W / 2, partial);
  AIR_CHECK_LAUNCH();
  hipLaunchKernelGGL(conv1_wgrad_final_kernel, dim3(nblk(C1_CO * (C1_TAPS + 1))), dim3(NT), 0, air_stream(stream),
                     partial, dw, db);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

int air_mfm_pool_fwd(const float* x, const float* bias, int B, int Ctot, int C, int H, int W, int pool, float* y,
                     uint8_t* route, air_stream_t stream) {
  if (!x || !y || !route || B <= 0 || C <= 0 || C % 2 || C > Ctot || H <= 0 || W <= 0) return AIR_EINVAL;
  if (pool && (H < 2 || W < 2)) return AIR_EINVAL;
  const int Ho = pool ? H / 2 : H, Wo = pool ? W / 2 : W;
  hipLaunchKernelGGL(mfm_pool_fwd_kernel, dim3(nblk((size_t)B * (C / 2) * Ho * Wo)), dim3(NT), 0, air_stream(stream),
                     x, bias, B, Ctot, C, H, W, pool ? 1 : 0, Ho, Wo, y, route);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

int air_mfm_pool_bwd(const float* dy, const uint8_t* route, int B, int Ctot, int C, int H, int W, int pool, float* dx,
                     air_stream_t stream) {
  if (!dy || !route || !dx || B <= 0 || C <= 0 || C % 2 || C > Ctot || H <= 0 || W <= 0) return AIR_EINVAL;
  if (pool && (H < 2 || W < 2)) return AIR_EINVAL;
  const int Ho = pool ? H / 2 : H, Wo = pool ? W / 2 : W;
  hipLaunchKernelGGL(mfm_pool_bwd_kernel, dim3(nblk((size_t)B * Ctot * H * W)), dim3(NT), 0, air_stream(stream), dy,
                     route, B, Ctot, C, H, W, pool ? 1 : 0, Ho, Wo, dx);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

int air_mfm_bias_grad(const float* dy, const uint8_t* route, int B, int C, int S, float* db, void* ws, size_t ws_bytes,
                      air_stream_t stream) {
  if (!dy || !route || !db || !ws || B <= 0 || C <= 0 || C % 2 || S <= 0) return AIR_EINVAL;
  if (ws_bytes < air_mfm_bias_grad_ws_bytes(C)) return AIR_EWORKSPACE;
  float* partial = static_cast<float*>(ws);
  hipLaunchKernelGGL(mfm_bias_partial_kernel, dim3(C / 2, BG_CHUNKS), dim3(NT), 0, air_stream(stream), dy, route, B,
                     C / 2, S, partial);
  AIR_CHECK_LAUNCH();
  hipLaunchKernelGGL(mfm_bias_final_kernel, dim3(nblk(C)), dim3(NT), 0, air_stream(stream), partial, C / 2, db);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

int air_copy_pad(float* dst, size_t n_dst, const float* src, size_t n_src, air_stream_t stream) {
  if (!dst || !src || n_dst == 0) return AIR_EINVAL;
  hipLaunchKernelGGL(copy_pad_kernel, dim3(nblk(n_dst)), dim3(NT), 0, air_stream(stream), dst, n_dst, src, n_src);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

int air_mul(const float* a, const float* b, size_t n, float* y, air_stream_t stream) {
  if (!a || !b || !y || n == 0) return AIR_EINVAL;
  hipLaunchKernelGGL(mul_kernel, dim3(nblk(n)), dim3(NT), 0, air_stream(stream), a, b, n, y);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

}  // extern "C"
