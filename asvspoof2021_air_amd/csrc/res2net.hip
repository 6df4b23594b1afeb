// SE-Res2Net-50 (model.py:256-509, main_train.py:169-170): the passes its blocks need beyond the convolutions
// (conv_narrow.hip, conv2d.hip), BatchNorm, row statistics and linear kernels.
//   * Res2 chain step with ReLU (model.py:461-470): y1 = relu(x*scale + shift) into a channel slice of the concat,
//     optionally y2 = y1 + add, the next branch's input "sp + spx[i+1]";
//   * AvgPool2d forward / backward on channel slices, PyTorch's window and divisor rules (ceil_mode,
//     count_include_pad): the stage block's 3x3 pool of its last split (model.py:442, :474) and the 2x2 ceil-mode
//     pool of the downsample path (model.py:294-298);
//   * SE tail (model.py:480-487, :499-505): out = relu(x*sigmoid(z[b][c]) + residual) and its backward;
//   * log_softmax over the (B, C) logits (model.py:353) and its backward.
// Sums run in a fixed order: the same bits on every run and replay.
#include "air_common.h"

namespace {

constexpr int NT = 256;

inline unsigned nblk(size_t n) { return (unsigned)((n + NT - 1) / NT); }

__global__ __launch_bounds__(NT) void res2_relu_kernel(const float* __restrict__ x, size_t xbs, int C, size_t S,
                                                       size_t n, const float* __restrict__ scale,
                                                       const float* __restrict__ shift, float* __restrict__ y1,
                                                       size_t y1bs, const float* __restrict__ add, size_t addbs,
                                                       float* __restrict__ y2) {
  const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  const size_t cs = (size_t)C * S;
  const size_t b = i / cs, r = i - b * cs;
  const int c = (int)(r / S);
  float v = x[b * xbs + r] * scale[c] + shift[c];
  v = fmaxf(v, 0.0f);
  y1[b * y1bs + r] = v;
  if (y2 != nullptr) y2[i] = v + add[b * addbs + r];
}

// PyTorch's avg_pool2d window (aten/src/ATen/native/AvgPool2d.cpp): [start, start + k) clipped to the padded input
// gives the count_include_pad divisor, clipped to the input the summed range and the other divisor.
struct PoolWin {
  int h0, h1, w0, w1;
  float div;
};

__device__ __forceinline__ PoolWin pool_win(int ho, int wo, int H, int W, int k, int s, int pad, int cip) {
  PoolWin q;
  int hs = ho * s - pad, ws = wo * s - pad;
  int he = min(hs + k, H + pad), we = min(ws + k, W + pad);
  const int full = (he - hs) * (we - ws);
  hs = max(hs, 0);
  ws = max(ws, 0);
  he = min(he, H);
  we = min(we, W);
  q.h0 = hs;
  q.h1 = he;
  q.w0 = ws;
  q.w1 = we;
  q.div = (float)(cip ? full : (he - hs) * (we - ws));
  return q;
}

__global__ __launch_bounds__(NT) void avgpool_fwd_kernel(const float* __restrict__ x, size_t xbs, int C, int H, int W,
                                                         int k, int s, int pad, int cip, int Ho, int Wo, size_t n,
                                                         float* __restrict__ y, size_t ybs) {
  const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  const int wo = (int)(i % Wo);
  const int ho = (int)((i / Wo) % Ho);
  const int c = (int)((i / ((size_t)Wo * Ho)) % C);
  const size_t b = i / ((size_t)Wo * Ho * C);
  const PoolWin q = pool_win(ho, wo, H, W, k, s, pad, cip);
  const float* xp = x + b * xbs + (size_t)c * H * W;
  float sum = 0.0f;
  for (int h = q.h0; h < q.h1; ++h)
    for (int w = q.w0; w < q.w1; ++w) sum += xp[(size_t)h * W + w];
  y[b * ybs + ((size_t)c * Ho + ho) * Wo + wo] = sum / q.div;
}

// Gather form of PyTorch's scatter backward: the windows that hold (h, w) in row-major order of the outputs, which
// is the order the scatter adds them in.
__global__ __launch_bounds__(NT) void avgpool_bwd_kernel(const float* __restrict__ dy, size_t dybs, int C, int H, int W,
                                                         int k, int s, int pad, int cip, int Ho, int Wo, size_t n,
                                                         float* __restrict__ dx, size_t dxbs, int accumulate) {
  const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  const int w = (int)(i % W);
  const int h = (int)((i / W) % H);
  const int c = (int)((i / ((size_t)W * H)) % C);
  const size_t b = i / ((size_t)W * H * C);
  // ho with ho*s - pad <= h < ho*s - pad + k
  const int ho0 = max(0, (h + pad - k + s) / s), ho1 = min(Ho - 1, (h + pad) / s);
  const int wo0 = max(0, (w + pad - k + s) / s), wo1 = min(Wo - 1, (w + pad) / s);
  const float* gp = dy + b * dybs + (size_t)c * Ho * Wo;
  float sum = 0.0f;
  for (int ho = ho0; ho <= ho1; ++ho)
    for (int wo = wo0; wo <= wo1; ++wo) {
      const PoolWin q = pool_win(ho, wo, H, W, k, s, pad, cip);
      if (h < q.h0 || h >= q.h1 || w < q.w0 || w >= q.w1) continue;
      sum += gp[(size_t)ho * Wo + wo] / q.div;
    }
  float* o = dx + b * dxbs + ((size_t)c * H + h) * W + w;
  *o = accumulate ? *o + sum : sum;
}

__device__ __forceinline__ float sigmoidf(float z) { return 1.0f / (1.0f + expf(-z)); }

__global__ __launch_bounds__(NT) void se_relu_fwd_kernel(const float* __restrict__ x, const float* __restrict__ z,
                                                         const float* __restrict__ res, size_t S, size_t n,
                                                         float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  const float g = sigmoidf(z[i / S]);
  out[i] = fmaxf(x[i] * g + res[i], 0.0f);
}

// One workgroup per (b, c) row: dpre = dout where out > 0; dx = dpre * g; dres = dpre; dz = g (1 - g) sum_s dpre x
// (each thread's strided sum, then the waves and the workgroup in a fixed order).
__global__ __launch_bounds__(NT) void se_relu_bwd_kernel(const float* __restrict__ x, const float* __restrict__ z,
                                                         const float* __restrict__ out, const float* __restrict__ dout,
                                                         size_t S, float* __restrict__ dx, float* __restrict__ dz,
                                                         float* __restrict__ dres) {
  __shared__ float red[NT / AIR_WAVE];
  const size_t row = blockIdx.x;
  const float g = sigmoidf(z[row]);
  const size_t base = row * S;
  float acc = 0.0f;
  for (size_t s = threadIdx.x; s < S; s += NT) {
    const size_t i = base + s;
    const float d = out[i] > 0.0f ? dout[i] : 0.0f;
    dx[i] = d * g;
    if (dres != nullptr) dres[i] = d;
    acc = fmaf(d, x[i], acc);
  }
  acc = air_wave_sum(acc);
  if ((threadIdx.x & (AIR_WAVE - 1)) == 0) red[threadIdx.x / AIR_WAVE] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = red[0];
#pragma unroll
    for (int q = 1; q < NT / AIR_WAVE; ++q) t += red[q];
    dz[row] = t * (g * (1.0f - g));
  }
}

__global__ __launch_bounds__(NT) void log_softmax_fwd_kernel(const float* __restrict__ zin, int B, int C,
                                                             float* __restrict__ out) {
  const int b = blockIdx.x * NT + threadIdx.x;
  if (b >= B) return;
  const float* zr = zin + (size_t)b * C;
  float m = zr[0];
  for (int c = 1; c < C; ++c) m = fmaxf(m, zr[c]);
  float s = 0.0f;
  for (int c = 0; c < C; ++c) s += expf(zr[c] - m);
  const float ls = logf(s);
  for (int c = 0; c < C; ++c) out[(size_t)b * C + c] = zr[c] - m - ls;
}

__global__ __launch_bounds__(NT) void log_softmax_bwd_kernel(const float* __restrict__ out,
                                                             const float* __restrict__ dout, int B, int C,
                                                             float* __restrict__ dz) {
  const int b = blockIdx.x * NT + threadIdx.x;
  if (b >= B) return;
  const size_t r = (size_t)b * C;
  float s = 0.0f;
  for (int c = 0; c < C; ++c) s += dout[r + c];
  for (int c = 0; c < C; ++c) dz[r + c] = dout[r + c] - expf(out[r + c]) * s;
}

int pool_out(int n, int k, int s, int pad, int ceil_mode) {
  const int num = n + 2 * pad - k;
  int o = (ceil_mode ? (num + s - 1) / s : num / s) + 1;
  if (ceil_mode && (o - 1) * s >= n + pad) --o;
  return o;
}

int pool_check(int B, int C, int H, int W, int k, int s, int pad, int ceil_mode, int Ho, int Wo) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || k <= 0 || s <= 0 || pad < 0 || 2 * pad > k) return AIR_EINVAL;
  if (Ho != pool_out(H, k, s, pad, ceil_mode) || Wo != pool_out(W, k, s, pad, ceil_mode) || Ho <= 0 || Wo <= 0)
    return AIR_EINVAL;
  return AIR_OK;
}

}  // namespace

extern "C" int air_res2_bn_relu_apply(const float* x, size_t x_bstride, int B, int C, int S, const float* scale,
                                      const float* shift, float* y1, size_t y1_bstride, const float* add,
                                      size_t add_bstride, float* y2, air_stream_t stream) {
  if (!x || !scale || !shift || !y1 || B <= 0 || C <= 0 || S <= 0) return AIR_EINVAL;
  if ((add == nullptr) != (y2 == nullptr)) return AIR_EINVAL;
  const size_t cs = (size_t)C * S;
  const size_t xbs = x_bstride ? x_bstride : cs, ybs = y1_bstride ? y1_bstride : cs,
               abs_ = add_bstride ? add_bstride : cs;
  if (xbs < cs || ybs < cs || abs_ < cs) return AIR_EINVAL;
  const size_t n = (size_t)B * cs;
  hipLaunchKernelGGL(res2_relu_kernel, dim3(nblk(n)), dim3(NT), 0, air_stream(stream), x, xbs, C, (size_t)S, n, scale,
                     shift, y1, ybs, add, abs_, y2);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

extern "C" int air_avgpool2d_fwd(const float* x, size_t x_bstride, int B, int C, int H, int W, int k, int stride,
                                 int pad, int ceil_mode, int count_include_pad, int Ho, int Wo, float* y,
                                 size_t y_bstride, air_stream_t stream) {
  if (!x || !y) return AIR_EINVAL;
  const int rc = pool_check(B, C, H, W, k, stride, pad, ceil_mode, Ho, Wo);
  if (rc != AIR_OK) return rc;
  const size_t xbs = x_bstride ? x_bstride : (size_t)C * H * W, ybs = y_bstride ? y_bstride : (size_t)C * Ho * Wo;
  if (xbs < (size_t)C * H * W || ybs < (size_t)C * Ho * Wo) return AIR_EINVAL;
  const size_t n = (size_t)B * C * Ho * Wo;
  hipLaunchKernelGGL(avgpool_fwd_kernel, dim3(nblk(n)), dim3(NT), 0, air_stream(stream), x, xbs, C, H, W, k, stride,
                     pad, count_include_pad, Ho, Wo, n, y, ybs);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

extern "C" int air_avgpool2d_bwd(const float* dy, size_t dy_bstride, int B, int C, int H, int W, int k, int stride,
                                 int pad, int ceil_mode, int count_include_pad, int Ho, int Wo, float* dx,
                                 size_t dx_bstride, int accumulate, air_stream_t stream) {
  if (!dy || !dx) return AIR_EINVAL;
  const int rc = pool_check(B, C, H, W, k, stride, pad, ceil_mode, Ho, Wo);
  if (rc != AIR_OK) return rc;
  const size_t dybs = dy_bstride ? dy_bstride : (size_t)C * Ho * Wo, dxbs = dx_bstride ? dx_bstride : (size_t)C * H * W;
  if (dxbs < (size_t)C * H * W || dybs < (size_t)C * Ho * Wo) return AIR_EINVAL;
  const size_t n = (size_t)B * C * H * W;
  hipLaunchKernelGGL(avgpool_bwd_kernel, dim3(nblk(n)), dim3(NT), 0, air_stream(stream), dy, dybs, C, H, W, k, stride,
                     pad, count_include_pad, Ho, Wo, n, dx, dxbs, accumulate);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

extern "C" int air_se_relu_fwd(const float* x, const float* z, const float* res, int B, int C, int S, float* out,
                               air_stream_t stream) {
  if (!x || !z || !res || !out || B <= 0 || C <= 0 || S <= 0) return AIR_EINVAL;
  const size_t n = (size_t)B * C * S;
  hipLaunchKernelGGL(se_relu_fwd_kernel, dim3(nblk(n)), dim3(NT), 0, air_stream(stream), x, z, res, (size_t)S, n, out);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

extern "C" int air_se_relu_bwd(const float* x, const float* z, const float* out, const float* dout, int B, int C, int S,
                               float* dx, float* dz, float* dres, air_stream_t stream) {
  if (!x || !z || !out || !dout || !dx || !dz || B <= 0 || C <= 0 || S <= 0) return AIR_EINVAL;
  hipLaunchKernelGGL(se_relu_bwd_kernel, dim3((unsigned)((size_t)B * C)), dim3(NT), 0, air_stream(stream), x, z, out,
                     dout, (size_t)S, dx, dz, dres);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

extern "C" int air_log_softmax_fwd(const float* z, int B, int C, float* out, air_stream_t stream) {
  if (!z || !out || B <= 0 || C <= 0) return AIR_EINVAL;
  hipLaunchKernelGGL(log_softmax_fwd_kernel, dim3(nblk((size_t)B)), dim3(NT), 0, air_stream(stream), z, B, C, out);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

extern "C" int air_log_softmax_bwd(const float* out, const float* dout, int B, int C, float* dz, air_stream_t stream) {
  if (!out || !dout || !dz || B <= 0 || C <= 0) return AIR_EINVAL;
  hipLaunchKernelGGL(log_softmax_bwd_kernel, dim3(nblk((size_t)B)), dim3(NT), 0, air_stream(stream), out, dout, B, C,
                     dz);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}
