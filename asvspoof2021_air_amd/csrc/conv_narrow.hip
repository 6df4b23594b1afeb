// Narrow-channel convolutions (SE-Res2Net-50, model.py:256-509): 3x3 pad 1 at stride 1 or 2 and 1x1 stride 1,
// 1 <= Cin, Cout <= 256 with ragged tails (the Res2 branches are 6, 13, 26 and 52 wide, the 1x1 layers 24 .. 256),
// fp32 NCHW.  The generic conv2d kernels tile 64 output channels and 8 input channels; padding these layers to that
// would multiply the work of the layer-1 branches (full 60 x 750 resolution) by tens.
//   * forward: one thread per output pixel and a tile of COT output channels in registers; the weights of a chunk of
//     input channels sit in LDS as [ci][tap][co] (wave-uniform broadcast reads).  Optional BatchNorm-apply + ReLU
//     prologue on the input (padding stays zero, as for the activated tensor);
//   * data gradient: one thread per input pixel and a tile of CIT input channels, weights as [co][tap][ci];
//   * weight gradient: a workgroup per (position chunk, 16 output channels, CIW input channels); each thread keeps
//     16 x CIW x taps sums over its positions, the workgroup folds them in a fixed order into a per-chunk partial
//     and a second kernel sums the chunks in index order: the same bits on every run and replay.
// Input, output and gradient may be channel slices of wider tensors: every tensor has a batch stride in elements.
#include "air_common.h"

namespace {

constexpr int NT = 256;
constexpr int WG_CO = 16;          // output channels per weight-gradient workgroup
constexpr int WG_MIN_POS = 8192;   // positions per weight-gradient chunk, at least
constexpr int WG_TARGET = 2048;    // weight-gradient workgroups aimed at

inline unsigned nblk(size_t n) { return (unsigned)((n + NT - 1) / NT); }

template <int K>
constexpr int ci_chunk() { return K == 3 ? 16 : 64; }

template <int K>
constexpr int wg_ci() { return K == 3 ? 1 : 8; }

__device__ __forceinline__ float act_in(float v, const float* __restrict__ sc, const float* __restrict__ sh, int ci,
                                        int relu) {
  if (sc != nullptr) {
    v = v * sc[ci] + sh[ci];
    if (relu) v = fmaxf(v, 0.0f);
  }
  return v;
}

// ------------------------------------------------------------------------------------------------- forward
template <int COT, int K, int S>
__global__ __launch_bounds__(NT) void narrow_fwd_kernel(const float* __restrict__ x, size_t xbs,
                                                        const float* __restrict__ w, const float* __restrict__ sc,
                                                        const float* __restrict__ sh, int relu, int B, int Cin, int H,
                                                        int W, int Cout, int Ho, int Wo, float* __restrict__ y,
                                                        size_t ybs) {
  constexpr int KK = K * K, P = K / 2, CH = ci_chunk<K>();
  __shared__ float sw[CH * KK * COT];
  const int co0 = blockIdx.y * COT;
  const size_t npix = (size_t)B * Ho * Wo;
  const size_t id = (size_t)blockIdx.x * NT + threadIdx.x;
  const bool valid = id < npix;
  const int wo = valid ? (int)(id % Wo) : 0;
  const int ho = valid ? (int)((id / Wo) % Ho) : 0;
  const int b = valid ? (int)(id / ((size_t)Wo * Ho)) : 0;
  float acc[COT];
#pragma unroll
  for (int j = 0; j < COT; ++j) acc[j] = 0.0f;
  const size_t plane = (size_t)H * W;
  for (int ci0 = 0; ci0 < Cin; ci0 += CH) {
    const int nci = Cin - ci0 < CH ? Cin - ci0 : CH;
    __syncthreads();
    for (int i = threadIdx.x; i < CH * KK * COT; i += NT) {
      const int j = i % COT, t = (i / COT) % KK, c = i / (COT * KK);
      const int co = co0 + j, ci = ci0 + c;
      sw[i] = (co < Cout && ci < Cin) ? w[((size_t)co * Cin + ci) * KK + t] : 0.0f;
    }
    __syncthreads();
    if (valid) {
#pragma unroll 1
      for (int c = 0; c < nci; ++c) {
        const int ci = ci0 + c;
        const float* xp = x + (size_t)b * xbs + (size_t)ci * plane;
#pragma unroll
        for (int kh = 0; kh < K; ++kh) {
          const int hi = ho * S - P + kh;
#pragma unroll
          for (int kw = 0; kw < K; ++kw) {
            const int wi = wo * S - P + kw;
            float v = 0.0f;
            if (hi >= 0 && hi < H && wi >= 0 && wi < W) v = act_in(xp[(size_t)hi * W + wi], sc, sh, ci, relu);
            const float* wr = sw + (c * KK + kh * K + kw) * COT;
#pragma unroll
            for (int j = 0; j < COT; ++j) acc[j] = fmaf(v, wr[j], acc[j]);
          }
        }
      }
    }
  }
  if (!valid) return;
  float* yp = y + (size_t)b * ybs + (size_t)ho * Wo + wo;
  const size_t oplane = (size_t)Ho * Wo;
#pragma unroll
  for (int j = 0; j < COT; ++j)
    if (co0 + j < Cout) yp[(size_t)(co0 + j) * oplane] = acc[j];
}

// ------------------------------------------------------------------------------------------- data gradient
template <int CIT, int K, int S>
__global__ __launch_bounds__(NT) void narrow_dgrad_kernel(const float* __restrict__ dy, size_t dybs,
                                                          const float* __restrict__ w, int B, int Cin, int H, int W,
                                                          int Cout, int Ho, int Wo, float* __restrict__ dx,
                                                          size_t dxbs, int accumulate) {
  constexpr int KK = K * K, P = K / 2, CH = ci_chunk<K>();
  __shared__ float sw[CH * KK * CIT];
  const int ci0 = blockIdx.y * CIT;
  const size_t npix = (size_t)B * H * W;
  const size_t id = (size_t)blockIdx.x * NT + threadIdx.x;
  const bool valid = id < npix;
  const int wi = valid ? (int)(id % W) : 0;
  const int hi = valid ? (int)((id / W) % H) : 0;
  const int b = valid ? (int)(id / ((size_t)W * H)) : 0;
  float acc[CIT];
#pragma unroll
  for (int j = 0; j < CIT; ++j) acc[j] = 0.0f;
  const size_t oplane = (size_t)Ho * Wo;
  for (int co0 = 0; co0 < Cout; co0 += CH) {
    const int nco = Cout - co0 < CH ? Cout - co0 : CH;
    __syncthreads();
    for (int i = threadIdx.x; i < CH * KK * CIT; i += NT) {
      const int j = i % CIT, t = (i / CIT) % KK, c = i / (CIT * KK);
      const int ci = ci0 + j, co = co0 + c;
      sw[i] = (co < Cout && ci < Cin) ? w[((size_t)co * Cin + ci) * KK + t] : 0.0f;
    }
    __syncthreads();
    if (valid) {
#pragma unroll 1
      for (int c = 0; c < nco; ++c) {
        const float* gp = dy + (size_t)b * dybs + (size_t)(co0 + c) * oplane;
#pragma unroll
        for (int kh = 0; kh < K; ++kh) {
          const int hn = hi + P - kh;
          const int ho = S == 1 ? hn : (hn >> 1);
          const bool hok = hn >= 0 && (S == 1 || (hn & 1) == 0) && ho < Ho;
#pragma unroll
          for (int kw = 0; kw < K; ++kw) {
            const int wn = wi + P - kw;
            const int wo = S == 1 ? wn : (wn >> 1);
            const bool ok = hok && wn >= 0 && (S == 1 || (wn & 1) == 0) && wo < Wo;
            const float g = ok ? gp[(size_t)ho * Wo + wo] : 0.0f;
            const float* wr = sw + (c * KK + kh * K + kw) * CIT;
#pragma unroll
            for (int j = 0; j < CIT; ++j) acc[j] = fmaf(g, wr[j], acc[j]);
          }
        }
      }
    }
  }
  if (!valid) return;
  float* xp = dx + (size_t)b * dxbs + (size_t)hi * W + wi;
  const size_t plane = (size_t)H * W;
#pragma unroll
  for (int j = 0; j < CIT; ++j) {
    if (ci0 + j < Cin) {
      float* o = xp + (size_t)(ci0 + j) * plane;
      *o = accumulate ? *o + acc[j] : acc[j];
    }
  }
}

// ----------------------------------------------------------------------------------------- weight gradient
struct WgPlan {
  int co_tiles, ci_tiles, chunks;
  size_t npos, per;
};

template <int K>
WgPlan wg_plan(const AirConvNarrow* p) {
  WgPlan q;
  q.co_tiles = (p->Cout + WG_CO - 1) / WG_CO;
  q.ci_tiles = (p->Cin + wg_ci<K>() - 1) / wg_ci<K>();
  q.npos = (size_t)p->B * p->Ho * p->Wo;
  const size_t by_size = (q.npos + WG_MIN_POS - 1) / WG_MIN_POS;
  const int others = q.co_tiles * q.ci_tiles;
  const size_t by_grid = (size_t)((WG_TARGET + others - 1) / others);
  size_t ch = by_size < by_grid ? by_size : by_grid;
  if (ch < 1) ch = 1;
  q.per = (q.npos + ch - 1) / ch;
  q.chunks = (int)((q.npos + q.per - 1) / q.per);
  return q;
}

template <int K, int S>
__global__ __launch_bounds__(NT) void narrow_wgrad_partial_kernel(const float* __restrict__ x, size_t xbs,
                                                                  const float* __restrict__ dy, size_t dybs,
                                                                  const float* __restrict__ sc,
                                                                  const float* __restrict__ sh, int relu, int B,
                                                                  int Cin, int H, int W, int Cout, int Ho, int Wo,
                                                                  size_t npos, size_t per,
                                                                  float* __restrict__ partial) {
  constexpr int KK = K * K, P = K / 2, CIW = wg_ci<K>(), NA = WG_CO * CIW * KK;
  __shared__ float red[NT / AIR_WAVE][NA];
  const int chunk = blockIdx.x, co0 = blockIdx.y * WG_CO, ci0 = blockIdx.z * CIW;
  const size_t lo = per * chunk;
  const size_t hi = lo + per < npos ? lo + per : npos;
  const size_t oplane = (size_t)Ho * Wo, plane = (size_t)H * W;
  float acc[WG_CO][CIW * KK];
#pragma unroll
  for (int j = 0; j < WG_CO; ++j)
#pragma unroll
    for (int k = 0; k < CIW * KK; ++k) acc[j][k] = 0.0f;
  for (size_t i = lo + threadIdx.x; i < hi; i += NT) {
    const int b = (int)(i / oplane);
    const size_t s = i - (size_t)b * oplane;
    const int ho = (int)(s / Wo), wo = (int)(s % Wo);
    float g[WG_CO];
    const float* gp = dy + (size_t)b * dybs + s;
#pragma unroll
    for (int j = 0; j < WG_CO; ++j) g[j] = co0 + j < Cout ? gp[(size_t)(co0 + j) * oplane] : 0.0f;
#pragma unroll
    for (int c = 0; c < CIW; ++c) {
      const int ci = ci0 + c;
      if (ci >= Cin) break;
      const float* xp = x + (size_t)b * xbs + (size_t)ci * plane;
#pragma unroll
      for (int kh = 0; kh < K; ++kh) {
        const int hh = ho * S - P + kh;
#pragma unroll
        for (int kw = 0; kw < K; ++kw) {
          const int ww = wo * S - P + kw;
          float v = 0.0f;
          if (hh >= 0 && hh < H && ww >= 0 && ww < W) v = act_in(xp[(size_t)hh * W + ww], sc, sh, ci, relu);
#pragma unroll
          for (int j = 0; j < WG_CO; ++j) acc[j][c * KK + kh * K + kw] = fmaf(g[j], v, acc[j][c * KK + kh * K + kw]);
        }
      }
    }
  }
  const int lane = threadIdx.x & (AIR_WAVE - 1), wave = threadIdx.x / AIR_WAVE;
#pragma unroll
  for (int j = 0; j < WG_CO; ++j)
#pragma unroll
    for (int k = 0; k < CIW * KK; ++k) {
      const float v = air_wave_sum(acc[j][k]);
      if (lane == 0) red[wave][j * CIW * KK + k] = v;
    }
  __syncthreads();
  const size_t wsz = (size_t)Cout * Cin * KK;
  for (int e = threadIdx.x; e < NA; e += NT) {
    const int j = e / (CIW * KK), r = e % (CIW * KK), c = r / KK, t = r % KK;
    const int co = co0 + j, ci = ci0 + c;
    if (co >= Cout || ci >= Cin) continue;
    float v = red[0][e];
#pragma unroll
    for (int q = 1; q < NT / AIR_WAVE; ++q) v += red[q][e];
    partial[(size_t)chunk * wsz + ((size_t)co * Cin + ci) * KK + t] = v;
  }
}

__global__ __launch_bounds__(NT) void narrow_wgrad_reduce_kernel(const float* __restrict__ partial, size_t wsz,
                                                                 int chunks, float* __restrict__ dw) {
  const size_t e = (size_t)blockIdx.x * NT + threadIdx.x;
  if (e >= wsz) return;
  float v = partial[e];
  for (int c = 1; c < chunks; ++c) v += partial[(size_t)c * wsz + e];
  dw[e] = v;
}

int check_desc(const AirConvNarrow* p) {
  if (!p || p->B <= 0 || p->H <= 0 || p->W <= 0) return AIR_EINVAL;
  if (p->Cin < 1 || p->Cout < 1) return AIR_EINVAL;
  if (p->Cin > 256 || p->Cout > 256) return AIR_EUNSUPPORTED;
  if (!((p->K == 3 && (p->stride == 1 || p->stride == 2)) || (p->K == 1 && p->stride == 1))) return AIR_EUNSUPPORTED;
  const int pad = p->K / 2;
  if (p->Ho != (p->H + 2 * pad - p->K) / p->stride + 1 || p->Wo != (p->W + 2 * pad - p->K) / p->stride + 1)
    return AIR_EINVAL;
  if (p->x_bstride != 0 && p->x_bstride < (size_t)p->Cin * p->H * p->W) return AIR_EINVAL;
  if (p->y_bstride != 0 && p->y_bstride < (size_t)p->Cout * p->Ho * p->Wo) return AIR_EINVAL;
  return AIR_OK;
}

size_t xbs_of(const AirConvNarrow* p) { return p->x_bstride ? p->x_bstride : (size_t)p->Cin * p->H * p->W; }
size_t ybs_of(const AirConvNarrow* p) { return p->y_bstride ? p->y_bstride : (size_t)p->Cout * p->Ho * p->Wo; }

template <int T, int K, int S>
void launch_fwd(const AirConvNarrow* p, const float* x, const float* w, const float* sc, const float* sh, int relu,
                float* y, hipStream_t st) {
  dim3 grid(nblk((size_t)p->B * p->Ho * p->Wo), (unsigned)((p->Cout + T - 1) / T));
  hipLaunchKernelGGL((narrow_fwd_kernel<T, K, S>), grid, dim3(NT), 0, st, x, xbs_of(p), w, sc, sh, relu, p->B, p->Cin,
                     p->H, p->W, p->Cout, p->Ho, p->Wo, y, ybs_of(p));
}

template <int T, int K, int S>
void launch_dgrad(const AirConvNarrow* p, const float* dy, const float* w, float* dx, int accumulate, hipStream_t st) {
  dim3 grid(nblk((size_t)p->B * p->H * p->W), (unsigned)((p->Cin + T - 1) / T));
  hipLaunchKernelGGL((narrow_dgrad_kernel<T, K, S>), grid, dim3(NT), 0, st, dy, ybs_of(p), w, p->B, p->Cin, p->H,
                     p->W, p->Cout, p->Ho, p->Wo, dx, xbs_of(p), accumulate);
}

// channel tile: the smallest of 8 / 16 / 32 that holds the count (the 6- and 13-wide branches waste little)
int tile_of(int c) { return c <= 8 ? 8 : (c <= 16 ? 16 : 32); }

}  // namespace

extern "C" int air_conv_narrow_fwd(const AirConvNarrow* p, const float* x, const float* w, const float* in_scale,
                                   const float* in_shift, int relu, float* y, air_stream_t stream) {
  const int rc = check_desc(p);
  if (rc != AIR_OK) return rc;
  if (!x || !w || !y || ((in_scale == nullptr) != (in_shift == nullptr))) return AIR_EINVAL;
  hipStream_t st = air_stream(stream);
  const int T = tile_of(p->Cout);
#define AIR_NARROW_FWD(TT)                                                                 \
  if (T == TT) {                                                                           \
    if (p->K == 1) launch_fwd<TT, 1, 1>(p, x, w, in_scale, in_shift, relu, y, st);          \
    else if (p->stride == 1) launch_fwd<TT, 3, 1>(p, x, w, in_scale, in_shift, relu, y, st); \
    else launch_fwd<TT, 3, 2>(p, x, w, in_scale, in_shift, relu, y, st);                    \
  }
  AIR_NARROW_FWD(8)
  AIR_NARROW_FWD(16)
  AIR_NARROW_FWD(32)
#undef AIR_NARROW_FWD
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

extern "C" int air_conv_narrow_dgrad(const AirConvNarrow* p, const float* dy, const float* w, float* dx,
                                     int accumulate, air_stream_t stream) {
  const int rc = check_desc(p);
  if (rc != AIR_OK) return rc;
  if (!dy || !w || !dx) return AIR_EINVAL;
  hipStream_t st = air_stream(stream);
  const int T = tile_of(p->Cin);
#define AIR_NARROW_DGRAD(TT)                                                   \
  if (T == TT) {                                                               \
    if (p->K == 1) launch_dgrad<TT, 1, 1>(p, dy, w, dx, accumulate, st);        \
    else if (p->stride == 1) launch_dgrad<TT, 3, 1>(p, dy, w, dx, accumulate, st); \
    else launch_dgrad<TT, 3, 2>(p, dy, w, dx, accumulate, st);                  \
  }
  AIR_NARROW_DGRAD(8)
  AIR_NARROW_DGRAD(16)
  AIR_NARROW_DGRAD(32)
#undef AIR_NARROW_DGRAD
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

extern "C" size_t air_conv_narrow_wgrad_ws_bytes(const AirConvNarrow* p) {
  if (check_desc(p) != AIR_OK) return 0;
  const WgPlan q = p->K == 3 ? wg_plan<3>(p) : wg_plan<1>(p);
  return (size_t)q.chunks * p->Cout * p->Cin * p->K * p->K * sizeof(float);
}

extern "C" int air_conv_narrow_wgrad(const AirConvNarrow* p, const float* x, const float* dy, const float* in_scale,
                                     const float* in_shift, int relu, float* dw, void* ws, size_t ws_bytes,
                                     air_stream_t stream) {
  const int rc = check_desc(p);
  if (rc != AIR_OK) return rc;
  if (!x || !dy || !dw || !ws || ((in_scale == nullptr) != (in_shift == nullptr))) return AIR_EINVAL;
  if (ws_bytes < air_conv_narrow_wgrad_ws_bytes(p)) return AIR_EWORKSPACE;
  hipStream_t st = air_stream(stream);
  float* part = static_cast<float*>(ws);
  const size_t wsz = (size_t)p->Cout * p->Cin * p->K * p->K;
  if (p->K == 1) {
    const WgPlan q = wg_plan<1>(p);
    hipLaunchKernelGGL((narrow_wgrad_partial_kernel<1, 1>), dim3(q.chunks, q.co_tiles, q.ci_tiles), dim3(NT), 0, st,
                       x, xbs_of(p), dy, ybs_of(p), in_scale, in_shift, relu, p->B, p->Cin, p->H, p->W, p->Cout, p->Ho,
                       p->Wo, q.npos, q.per, part);
    AIR_CHECK_LAUNCH();
    hipLaunchKernelGGL(narrow_wgrad_reduce_kernel, dim3(nblk(wsz)), dim3(NT), 0, st, part, wsz, q.chunks, dw);
  } else {
    const WgPlan q = wg_plan<3>(p);
    if (p->stride == 1)
      hipLaunchKernelGGL((narrow_wgrad_partial_kernel<3, 1>), dim3(q.chunks, q.co_tiles, q.ci_tiles), dim3(NT), 0, st,
                         x, xbs_of(p), dy, ybs_of(p), in_scale, in_shift, relu, p->B, p->Cin, p->H, p->W, p->Cout,
                         p->Ho, p->Wo, q.npos, q.per, part);
    else
      hipLaunchKernelGGL((narrow_wgrad_partial_kernel<3, 2>), dim3(q.chunks, q.co_tiles, q.ci_tiles), dim3(NT), 0, st,
                         x, xbs_of(p), dy, ybs_of(p), in_scale, in_shift, relu, p->B, p->Cin, p->H, p->W, p->Cout,
                         p->Ho, p->Wo, q.npos, q.per, part);
    AIR_CHECK_LAUNCH();
    hipLaunchKernelGGL(narrow_wgrad_reduce_kernel, dim3(nblk(wsz)), dim3(NT), 0, st, part, wsz, q.chunks, dw);
  }
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}
