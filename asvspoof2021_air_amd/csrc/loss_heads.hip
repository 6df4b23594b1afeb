// The reference's other loss heads for gfx950, one launch per pass each (the pattern of ocsoftmax.hip: one
// workgroup, a wave per row with RU rows in flight, per-row terms through LDS summed in a fixed row order, no
// atomics - graph replay == eager, bit for bit):
//   P2SGradLoss (loss.py:244-335)                      forward + backward (dx, dweight)
//   IsolateLoss / IsolateSquareLoss (loss.py:99-173)   forward + backward (dx, dcenter), one kernel pair with a flag
//   AMSoftmax (loss.py:209-234)                        forward only (the reference only scores with it)
#include "air_common.h"

namespace {

constexpr int NT = 1024;
constexpr int NW = NT / 64;
constexpr int MAXB = 4096;
constexpr int MAXC = 4;     // P2SGrad classes (the reference builds it with 2: main_train.py:274-277)
constexpr int MAXD = 1024;  // P2SGrad feature dimension (its weight gradient is staged in LDS)
constexpr int RU = 4;

// dimension chunk of the backward passes: DC = D rounded up to a power of two in [64, NT]; NT / DC row groups
__device__ __forceinline__ int chunk_cols(int D) {
  int DC = 64;
  while (DC < D && DC < NT) DC <<= 1;
  return DC;
}

// ------------------------------------------------------------------------------------------------------- P2SGrad
// w = weight.renorm(2, 1, 1e-5).mul(1e5): column j scaled by f_j = 1e-5 / (|W_j| + 1e-7) where |W_j| > 1e-5
__device__ __forceinline__ void p2s_col_norms(const float* __restrict__ W, int D, int C, int lane, float (&n)[MAXC],
                                              float (&f)[MAXC]) {
#pragma unroll
  for (int j = 0; j < MAXC; ++j) n[j] = 0.0f;
  for (int d = lane; d < D; d += 64) {
#pragma unroll
    for (int j = 0; j < MAXC; ++j)
      if (j < C) n[j] = fmaf(W[(size_t)d * C + j], W[(size_t)d * C + j], n[j]);
  }
#pragma unroll
  for (int j = 0; j < MAXC; ++j) {
    n[j] = sqrtf(air_wave_sum(n[j]));
    f[j] = n[j] > 1e-5f ? 1e-5f / (n[j] + 1e-7f) : 1.0f;
  }
}

// |x_b|^2 and x_b . w_j of RU rows (w from W on the fly)
__device__ __forceinline__ void p2s_row_dots(const float* __restrict__ x, const float* __restrict__ W, int B, int D,
                                             int C, const float (&f)[MAXC], int b0, int lane, float (&xx)[RU],
                                             float (&xw)[RU][MAXC]) {
#pragma unroll
  for (int u = 0; u < RU; ++u) {
    xx[u] = 0.0f;
#pragma unroll
    for (int j = 0; j < MAXC; ++j) xw[u][j] = 0.0f;
  }
  for (int d = lane; d < D; d += 64) {
    float w[MAXC];
#pragma unroll
    for (int j = 0; j < MAXC; ++j) w[j] = j < C ? (W[(size_t)d * C + j] * f[j]) * 1e5f : 0.0f;
    float v[RU];
#pragma unroll
    for (int u = 0; u < RU; ++u) v[u] = b0 + u * NW < B ? x[(size_t)(b0 + u * NW) * D + d] : 0.0f;
#pragma unroll
    for (int u = 0; u < RU; ++u) {
      xx[u] = fmaf(v[u], v[u], xx[u]);
#pragma unroll
      for (int j = 0; j < MAXC; ++j) xw[u][j] = fmaf(v[u], w[j], xw[u][j]);
    }
  }
#pragma unroll
  for (int u = 0; u < RU; ++u) {
    xx[u] = air_wave_sum(xx[u]);
#pragma unroll
    for (int j = 0; j < MAXC; ++j) xw[u][j] = air_wave_sum(xw[u][j]);
  }
}

__device__ __forceinline__ float p2s_target(int j, int64_t label, int C, float smooth) {
  return (j == (int)label ? 1.0f : 0.0f) * (1.0f - smooth) + smooth / (float)C;  // smooth_labels (loss.py:291-297)
}

__global__ __launch_bounds__(NT) void p2s_fwd_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                     const int64_t* __restrict__ labels, int B, int D, int C,
                                                     float smooth, float* __restrict__ loss,
                                                     float* __restrict__ neg_cos0) {
  __shared__ float s_t[MAXB];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float n[MAXC], f[MAXC];
  p2s_col_norms(W, D, C, lane, n, f);
  for (int b0 = wave; b0 < B; b0 += NW * RU) {
    float xx[RU], xw[RU][MAXC];
    p2s_row_dots(x, W, B, D, C, f, b0, lane, xx, xw);
#pragma unroll
    for (int u = 0; u < RU; ++u) {
      const int b = b0 + u * NW;
      if (b < B && lane == 0) {
        const float xm = sqrtf(xx[u]);  // no epsilon (loss.py:314)
        const int64_t lab = labels[b];
        float t = 0.0f;
#pragma unroll
        for (int j = 0; j < MAXC; ++j) {
          if (j < C) {
            const float cu = xw[u][j] / xm;
            const float cs = cu != cu ? cu : fminf(fmaxf(cu, -1.0f), 1.0f);  // torch's clamp keeps a NaN
            const float e = cs - p2s_target(j, lab, C, smooth);
            t = fmaf(e, e, t);
            if (j == 0) neg_cos0[b] = -cs;
          }
        }
        s_t[b] = t;
      }
    }
  }
  __syncthreads();
  if (wave == 0) {
    float t = 0.0f;
    for (int b = lane; b < B; b += 64) t += s_t[b];
    t = air_wave_sum(t);
    if (lane == 0) loss[0] = t / (float)(B * C);  // nn.MSELoss: mean over B x C
  }
}

// phase 1: per-row k_bj = dL/dcos (0 where the clamp cut), 1/|x| and a_b = sum_j k_bj cos_bj (unclamped) into LDS;
// phase 2: dx elementwise, the gradient of w summed over rows per (d, j) through LDS in a fixed order;
// phase 3: per column, renorm's backward (torch's renorm_backward: scale and column-norm term) and the 1e5 factor
__global__ __launch_bounds__(NT) void p2s_bwd_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                     const int64_t* __restrict__ labels, int B, int D, int C,
                                                     float smooth, const float* __restrict__ gscale,
                                                     float* __restrict__ dx, float* __restrict__ dW) {
  __shared__ float s_k[MAXB * MAXC], s_inv[MAXB], s_a[MAXB];
  __shared__ float s_part[NT];
  __shared__ float s_gw[MAXD * MAXC];
  __shared__ float s_dot[MAXC];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float n[MAXC], f[MAXC];
  p2s_col_norms(W, D, C, lane, n, f);
  const float g0 = gscale ? gscale[0] : 1.0f;
  const float sc = 2.0f * g0 / (float)(B * C);
  for (int b0 = wave; b0 < B; b0 += NW * RU) {
    float xx[RU], xw[RU][MAXC];
    p2s_row_dots(x, W, B, D, C, f, b0, lane, xx, xw);
#pragma unroll
    for (int u = 0; u < RU; ++u) {
      const int b = b0 + u * NW;
      if (b < B && lane == 0) {
        const float xm = sqrtf(xx[u]);
        const int64_t lab = labels[b];
        float a = 0.0f;
#pragma unroll
        for (int j = 0; j < MAXC; ++j) {
          if (j < C) {
            const float cu = xw[u][j] / xm;
            const float cs = cu != cu ? cu : fminf(fmaxf(cu, -1.0f), 1.0f);
            // clamp's backward passes the gradient where -1 <= cos <= 1 (NaN compares false: no gradient)
            const float k = (cu >= -1.0f && cu <= 1.0f) ? sc * (cs - p2s_target(j, lab, C, smooth)) : 0.0f;
            s_k[b * MAXC + j] = k;
            a = fmaf(k, cu, a);
          }
        }
        s_inv[b] = 1.0f / xm;
        s_a[b] = a;
      }
    }
  }
  __syncthreads();
  const int DC = chunk_cols(D);
  const int G = NT / DC, dl = threadIdx.x % DC, g = threadIdx.x / DC;
  for (int j = 0; j < C; ++j) {
    for (int d0 = 0; d0 < D; d0 += DC) {
      const int d = d0 + dl;
      float gw = 0.0f;
      if (d < D) {
        for (int b = g; b < B; b += G * RU) {
          float v[RU];
#pragma unroll
          for (int u = 0; u < RU; ++u) v[u] = b + u * G < B ? x[(size_t)(b + u * G) * D + d] : 0.0f;
#pragma unroll
          for (int u = 0; u < RU; ++u) {
            const int bb = b + u * G;
            if (bb < B) gw = fmaf(s_k[bb * MAXC + j], v[u] * s_inv[bb], gw);  // d(inner / |x|) / dw
          }
        }
      }
      s_part[threadIdx.x] = gw;
      __syncthreads();
      if (g == 0 && d < D) {
        float t = 0.0f;
        for (int q = 0; q < G; ++q) t += s_part[q * DC + dl];
        s_gw[d * MAXC + j] = t * 1e5f;  // through .mul(1e5)
      }
      __syncthreads();
    }
  }
  // dx_bd = (sum_j k_bj w_dj - a_b x_bd / |x_b|) / |x_b|
  for (int i = threadIdx.x; i < B * D; i += NT) {
    const int b = i / D, d = i - b * D;
    float s = 0.0f;
    for (int j = 0; j < C; ++j) s = fmaf(s_k[b * MAXC + j], (W[(size_t)d * C + j] * f[j]) * 1e5f, s);
    const float inv = s_inv[b];
    dx[i] = (s - s_a[b] * x[i] * inv) * inv;
  }
  // <W_j, g_j> per column: wave j, lanes over d, one wave sum
  if (wave < C) {
    float t = 0.0f;
    for (int d = lane; d < D; d += 64) t = fmaf(W[(size_t)d * C + wave], s_gw[d * MAXC + wave], t);
    t = air_wave_sum(t);
    if (lane == 0) s_dot[wave] = t;
  }
  __syncthreads();
  // renorm_backward: where |W_j| > maxnorm: f g - (f / (|W_j| + 1e-7)) (<W_j, g> / |W_j|) W_j; else g
  for (int i = threadIdx.x; i < D * C; i += NT) {
    const int d = i / C, j = i - d * C;
    const float gv = s_gw[d * MAXC + j];
    if (n[j] > 1e-5f) {
      const float inv = 1.0f / (n[j] + 1e-7f);
      dW[i] = f[j] * gv - (f[j] * inv) * (s_dot[j] / n[j] * W[i]);
    } else {
      dW[i] = gv;
    }
  }
}

// ------------------------------------------------------------------------------------------------------- Isolate
// |x_b - c|^2 of RU rows
__device__ __forceinline__ void iso_row_dist(const float* __restrict__ x, const float* __restrict__ c, int B, int D,
                                             int b0, int lane, float (&dd)[RU]) {
#pragma unroll
  for (int u = 0; u < RU; ++u) dd[u] = 0.0f;
  for (int d = lane; d < D; d += 64) {
    const float cd = c[d];
    float v[RU];
#pragma unroll
    for (int u = 0; u < RU; ++u) v[u] = b0 + u * NW < B ? x[(size_t)(b0 + u * NW) * D + d] - cd : 0.0f;
#pragma unroll
    for (int u = 0; u < RU; ++u) dd[u] = fmaf(v[u], v[u], dd[u]);
  }
#pragma unroll
  for (int u = 0; u < RU; ++u) dd[u] = air_wave_sum(dd[u]);
}

// the ReLU input of row b: label 0: |x - c| - r_real (square: |x - c|^2 - r_real^2); label 1: r_fake - |x - c| (...)
__device__ __forceinline__ float iso_arg(float nrm, bool real, float r_real, float r_fake, int square) {
  const float q = square ? nrm * nrm : nrm;
  return real ? q - r_real : r_fake - q;
}

// the row counts of both classes (every wave alike; B <= 4096 labels)
__device__ __forceinline__ void iso_counts(const int64_t* __restrict__ labels, int B, int lane, int& n0, int& n1) {
  float c0 = 0.0f, c1 = 0.0f;
  for (int b = lane; b < B; b += 64) {
    const int64_t l = labels[b];
    c0 += l == 0 ? 1.0f : 0.0f;
    c1 += l == 1 ? 1.0f : 0.0f;
  }
  n0 = (int)air_wave_sum(c0);
  n1 = (int)air_wave_sum(c1);
}

// dist (optional): |x_b - c|, the dev-pass score of main_train.py:548
// loss = mean over label-0 rows of relu(arg) + mean over label-1 rows (0 / 0 = NaN for an absent class, as torch's
// mean of an empty tensor).  r_real / r_fake arrive squared for IsolateSquareLoss.
__global__ __launch_bounds__(NT) void iso_fwd_kernel(const float* __restrict__ x, const float* __restrict__ c,
                                                     const int64_t* __restrict__ labels, int B, int D, float r_real,
                                                     float r_fake, int square, float* __restrict__ loss,
                                                     float* __restrict__ dist) {
  __shared__ float s_t[MAXB];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int b0 = wave; b0 < B; b0 += NW * RU) {
    float dd[RU];
    iso_row_dist(x, c, B, D, b0, lane, dd);
#pragma unroll
    for (int u = 0; u < RU; ++u) {
      const int b = b0 + u * NW;
      if (b < B && lane == 0) {
        const int64_t l = labels[b];
        const float nrm = sqrtf(dd[u]);
        s_t[b] = (l == 0 || l == 1) ? fmaxf(iso_arg(nrm, l == 0, r_real, r_fake, square), 0.0f) : 0.0f;
        if (dist) dist[b] = nrm;
      }
    }
  }
  __syncthreads();
  if (wave == 0) {
    float t0 = 0.0f, t1 = 0.0f, c0 = 0.0f, c1 = 0.0f;
    for (int b = lane; b < B; b += 64) {
      const int64_t l = labels[b];
      if (l == 0) { t0 += s_t[b]; c0 += 1.0f; }
      if (l == 1) { t1 += s_t[b]; c1 += 1.0f; }
    }
    t0 = air_wave_sum(t0);
    t1 = air_wave_sum(t1);
    c0 = air_wave_sum(c0);
    c1 = air_wave_sum(c1);
    if (lane == 0) loss[0] = t0 / c0 + t1 / c1;
  }
}

// phase 1: per-row coefficient q_b of (x_b - c) into LDS; phase 2: dx elementwise, dcenter = -sum_b q_b (x_b - c)
// over row groups through LDS in a fixed order.  Norm gradient 0 at |x - c| == 0; a ReLU input of exactly 0 passes none.
__global__ __launch_bounds__(NT) void iso_bwd_kernel(const float* __restrict__ x, const float* __restrict__ c,
                                                     const int64_t* __restrict__ labels, int B, int D, float r_real,
                                                     float r_fake, int square, const float* __restrict__ gscale,
                                                     float* __restrict__ dx, float* __restrict__ dc) {
  __shared__ float s_q[MAXB];
  __shared__ float s_part[NT];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float g0 = gscale ? gscale[0] : 1.0f;
  int n0, n1;
  iso_counts(labels, B, lane, n0, n1);
  for (int b0 = wave; b0 < B; b0 += NW * RU) {
    float dd[RU];
    iso_row_dist(x, c, B, D, b0, lane, dd);
#pragma unroll
    for (int u = 0; u < RU; ++u) {
      const int b = b0 + u * NW;
      if (b < B && lane == 0) {
        const int64_t l = labels[b];
        const float nrm = sqrtf(dd[u]);
        float q = 0.0f;
        if ((l == 0 || l == 1) && iso_arg(nrm, l == 0, r_real, r_fake, square) > 0.0f && nrm != 0.0f) {
          const float k = l == 0 ? g0 / (float)n0 : -g0 / (float)n1;  // d(loss) / d(|x - c|) (or of its square)
          q = square ? (k * (2.0f * nrm)) / nrm : k / nrm;
        }
        s_q[b] = q;
      }
    }
  }
  __syncthreads();
  const int DC = chunk_cols(D);
  const int G = NT / DC, dl = threadIdx.x % DC, g = threadIdx.x / DC;
  for (int d0 = 0; d0 < D; d0 += DC) {
    const int d = d0 + dl;
    float gc = 0.0f;
    if (d < D) {
      const float cd = c[d];
      for (int b = g; b < B; b += G * RU) {
        float v[RU];
#pragma unroll
        for (int u = 0; u < RU; ++u) v[u] = b + u * G < B ? x[(size_t)(b + u * G) * D + d] - cd : 0.0f;
#pragma unroll
        for (int u = 0; u < RU; ++u) {
          const int bb = b + u * G;
          if (bb < B) {
            const float t = s_q[bb] * v[u];
            dx[(size_t)bb * D + d] = t;
            gc += t;
          }
        }
      }
    }
    s_part[threadIdx.x] = gc;
    __syncthreads();
    if (g == 0 && d < D) {
      float t = 0.0f;
      for (int q = 0; q < G; ++q) t += s_part[q * DC + dl];
      dc[d] = -t;
    }
    __syncthreads();
  }
}

// ----------------------------------------------------------------------------------------------------- AMSoftmax
// logits_bj = <x_b / |x_b|, c_j / |c_j|>; margin_bj = s (logits_bj - m [j == label_b]).  A wave per (row, class).
__global__ __launch_bounds__(NT) void ams_fwd_kernel(const float* __restrict__ x, const float* __restrict__ centers,
                                                     const int64_t* __restrict__ labels, int B, int D, int C, float s,
                                                     float m, float* __restrict__ logits,
                                                     float* __restrict__ margin) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = wave; i < B * C; i += NW) {
    const int b = i / C, j = i - b * C;
    float xx = 0.0f, cc = 0.0f, xc = 0.0f;
    for (int d = lane; d < D; d += 64) {
      const float v = x[(size_t)b * D + d], w = centers[(size_t)j * D + d];
      xx = fmaf(v, v, xx);
      cc = fmaf(w, w, cc);
      xc = fmaf(v, w, xc);
    }
    xx = air_wave_sum(xx);
    cc = air_wave_sum(cc);
    xc = air_wave_sum(xc);
    if (lane == 0) {
      const float lg = xc / (sqrtf(xx) * sqrtf(cc));  // no epsilon (loss.py:218-223)
      logits[i] = lg;
      margin[i] = s * (lg - (j == (int)labels[b] ? m : 0.0f));
    }
  }
}

}  // namespace

extern "C" {

int air_p2sgrad_fwd(const float* x, const float* weight, const int64_t* labels, int B, int D, int C, float smooth,
                    float* loss, float* neg_cos0, air_stream_t stream) {
  if (!x || !weight || !labels || !loss || !neg_cos0 || B <= 0 || D <= 0 || C <= 0) return AIR_EINVAL;
  if (B > MAXB || C > MAXC || D > MAXD) return AIR_EUNSUPPORTED;
  hipLaunchKernelGGL(p2s_fwd_kernel, dim3(1), dim3(NT), 0, air_stream(stream), x, weight, labels, B, D, C, smooth,
                     loss, neg_cos0);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

int air_p2sgrad_bwd(const float* x, const float* weight, const int64_t* labels, int B, int D, int C, float smooth,
                    const float* gscale_dev, float* dx, float* dweight, air_stream_t stream) {
  if (!x || !weight || !labels || !dx || !dweight || B <= 0 || D <= 0 || C <= 0) return AIR_EINVAL;
  if (B > MAXB || C > MAXC || D > MAXD) return AIR_EUNSUPPORTED;
  hipLaunchKernelGGL(p2s_bwd_kernel, dim3(1), dim3(NT), 0, air_stream(stream), x, weight, labels, B, D, C, smooth,
                     gscale_dev, dx, dweight);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

int air_isolate_fwd(const float* x, const float* center, const int64_t* labels, int B, int D, float r_real,
                    float r_fake, int square, float* loss, float* dist_or_null, air_stream_t stream) {
  if (!x || !center || !labels || !loss || B <= 0 || D <= 0) return AIR_EINVAL;
  if (B > MAXB) return AIR_EUNSUPPORTED;
  hipLaunchKernelGGL(iso_fwd_kernel, dim3(1), dim3(NT), 0, air_stream(stream), x, center, labels, B, D, r_real, r_fake,
                     square, loss, dist_or_null);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

int air_isolate_bwd(const float* x, const float* center, const int64_t* labels, int B, int D, float r_real,
                    float r_fake, int square, const float* gscale_dev, float* dx, float* dcenter,
                    air_stream_t stream) {
  if (!x || !center || !labels || !dx || !dcenter || B <= 0 || D <= 0) return AIR_EINVAL;
  if (B > MAXB) return AIR_EUNSUPPORTED;
  hipLaunchKernelGGL(iso_bwd_kernel, dim3(1), dim3(NT), 0, air_stream(stream), x, center, labels, B, D, r_real, r_fake,
                     square, gscale_dev, dx, dcenter);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

int air_amsoftmax_fwd(const float* x, const float* centers, const int64_t* labels, int B, int D, int C, float s,
                      float m, float* logits, float* margin_logits, air_stream_t stream) {
  if (!x || !centers || !labels || !logits || !margin_logits || B <= 0 || D <= 0 || C <= 0) return AIR_EINVAL;
  if (B > MAXB) return AIR_EUNSUPPORTED;
  hipLaunchKernelGGL(ams_fwd_kernel, dim3(1), dim3(NT), 0, air_stream(stream), x, centers, labels, B, D, C, s, m,
                     logits, margin_logits);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

}  // extern "C"
