// Adversarial channel-classifier head: the small kernels around the two
// nn.Linear layers of model.ChannelClassifier (model.py:1007-1023) and nn.CrossEntropyLoss
// (main_train.py:251, :386, :396-397, :428, :446-450).  All latency-class: B <= a few hundred
// rows of <= 128 floats.
#include <cstdint>

#include "air_common.h"
#include "air_philox.h"

namespace {

constexpr int NT = 256;

// nn.Dropout(p) keep-mask, already scaled: keep = (u >= p) / (1 - p), u ~ U[0,1) from Philox4x32-10.  One body for
// the host-offset draw, the device-counter draw (air_dropout_mask_ctr) and the draw inside the fused heads
// (air_adv_heads), so that the three cannot drift apart: quad q of the flattened mask is Philox(seed, offset + q).
__device__ __forceinline__ void dropout_quad(float* keep, size_t n, float p, uint64_t seed, uint64_t offset,
                                             size_t quad) {
  if (quad * 4 >= n) return;
  uint32_t c[4];
  air_philox_block(offset + quad, seed, c);
  const float scale = 1.0f / (1.0f - p);
  for (int j = 0; j < 4; ++j)
    if (quad * 4 + j < n) keep[quad * 4 + j] = (air_philox_u01(c[j]) >= p) ? scale : 0.0f;
}
__device__ __forceinline__ void dropout_body(float* __restrict__ keep, size_t n, float p, uint64_t seed,
                                             uint64_t offset) {
  dropout_quad(keep, n, p, seed, offset, (size_t)blockIdx.x * NT + threadIdx.x);
}

__global__ __launch_bounds__(NT) void dropout_mask_kernel(float* __restrict__ keep, size_t n, float p,
                                                          uint64_t seed, uint64_t offset) {
  dropout_body(keep, n, p, seed, offset);
}

// The same draw with the Philox offset read from device memory, and the 1-thread kernel that advances it behind the
// draw (a captured hipGraph would freeze a host-side offset)
__global__ __launch_bounds__(NT) void dropout_mask_ctr_kernel(float* __restrict__ keep, size_t n, float p,
                                                              uint64_t seed,
                                                              const unsigned long long* __restrict__ counter) {
  dropout_body(keep, n, p, seed, (uint64_t)*counter);
}
__global__ void dropout_ctr_add_kernel(unsigned long long* counter, unsigned long long inc) { *counter += inc; }

// y = relu(x * keep)   (Dropout -> ReLU, model.py:1013-1014; keep NULL in eval mode)
__global__ __launch_bounds__(NT) void mask_relu_fwd_kernel(const float* __restrict__ x, const float* __restrict__ keep,
                                                           size_t n, float* __restrict__ y) {
  const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
  if (i < n) y[i] = fmaxf(keep ? x[i] * keep[i] : x[i], 0.0f);
}

// dx = alpha * dy * keep * (y > 0)
__global__ __launch_bounds__(NT) void mask_relu_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                           const float* __restrict__ keep, size_t n, float alpha,
                                                           float* __restrict__ dx) {
  const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
  if (i < n) dx[i] = y[i] > 0.0f ? alpha * dy[i] * (keep ? keep[i] : 1.0f) : 0.0f;
}

__global__ __launch_bounds__(NT) void scale_kernel(float* __restrict__ x, size_t n, float alpha) {
  const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
  if (i < n) x[i] *= alpha;
}

// One workgroup: probs = softmax(logits) per row, loss = mean_b -log probs[b][label[b]], plus the
// count of rows whose argmax equals the label (the accuracy counters of main_train.py:383-385).
__global__ __launch_bounds__(NT) void softmax_ce_fwd_kernel(const float* __restrict__ logits,
                                                            const long long* __restrict__ labels, int B, int C,
                                                            float* __restrict__ probs, float* __restrict__ loss,
                                                            int* __restrict__ correct) {
  __shared__ double sh[NT / 64];
  __shared__ int shc[NT / 64];
  double acc = 0.0;
  int hit = 0;
  for (int b = threadIdx.x; b < B; b += NT) {
    const float* __restrict__ row = logits + (size_t)b * C;
    float m = row[0];
    int am = 0;
    for (int c = 1; c < C; ++c)
      if (row[c] > m) { m = row[c]; am = c; }  // first maximum, like torch.max
    // the row sum in double: with a sequential fp32 sum the probabilities of a (700, 128) batch were up to 5.3e-7
    // off an fp64 softmax on the device, against the 4 * 2^-24 = 2.4e-7 they are held to
    double sd = 0.0;
    for (int c = 0; c < C; ++c) sd += (double)expf(row[c] - m);
    const float s = (float)sd;
    const float inv = (float)(1.0 / sd);
    for (int c = 0; c < C; ++c) probs[(size_t)b * C + c] = expf(row[c] - m) * inv;
    const int lab = (int)labels[b];
    acc += (double)(logf(s) - (row[lab] - m));
    hit += am == lab;
  }
  acc = air_wave_sum_d(acc);
  for (int o = 32; o > 0; o >>= 1) hit += __shfl_xor(hit, o, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { sh[wave] = acc; shc[wave] = hit; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    int h = 0;
    for (int w = 0; w < NT / 64; ++w) { t += sh[w]; h += shc[w]; }
    *loss = (float)(t / B);
    if (correct) *correct = h;
  }
}

// dlogits[b][c] = g * (probs[b][c] - [c == label[b]]) / B
__global__ __launch_bounds__(NT) void softmax_ce_bwd_kernel(const float* __restrict__ probs,
                                                            const long long* __restrict__ labels, int B, int C,
                                                            const float* __restrict__ gscale, float* __restrict__ dlogits) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= B * C) return;
  const int b = i / C, c = i - b * C;
  const float g = (gscale ? *gscale : 1.0f) / (float)B;
  dlogits[i] = g * (probs[i] - (c == (int)labels[b] ? 1.0f : 0.0f));
}

// ---------------------------------------------------------------------------------------------------------------
// air_adv_heads: every classifier head of one phase in one launch, one workgroup per head.  The six small products
// of a head (h, logits, dw2, dh, dw1, dx) run on one LDS-tiled routine; the intermediates (h, the mask factor, the
// logits) live in a scratch buffer that only this workgroup touches, ordered by workgroup barriers.
constexpr int FT = 64;   // output tile (FT x FT), 4 x 4 per thread
constexpr int FK = 16;   // reduction chunk staged through LDS

struct FusedLds {
  float a[FK][FT + 4];  // (+4: rows stay 16-byte aligned, and the k-contiguous loads scatter over the banks)
  float b[FK][FT + 4];
};

// out(m, n) = sum_k A[m * sam + k * sak] * Bm[n * sbn + k * sbk], k ascending in one fp32 fmaf chain per output;
// epi(m, n, sum) stores it.  The next chunk's global loads are in flight while the current one is multiplied.
// M, N, K and the strides are workgroup-uniform (barriers inside).
template <class Epi>
__device__ __forceinline__ void tile_gemm(FusedLds& s, const float* A, size_t sam, size_t sak, const float* Bm,
                                          size_t sbn, size_t sbk, int M, int N, int K, Epi epi) {
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
  const bool akc = sak == 1, bkc = sbk == 1;
  for (int m0 = 0; m0 < M; m0 += FT)
    for (int n0 = 0; n0 < N; n0 += FT) {
      float acc[4][4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0f;
      float ra[4], rb[4];
      auto fetch = [&](int k0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int e = t + r * NT;
          const int ka = akc ? (e & (FK - 1)) : (e >> 6), ma = akc ? (e >> 4) : (e & (FT - 1));
          const int kb = bkc ? (e & (FK - 1)) : (e >> 6), nb = bkc ? (e >> 4) : (e & (FT - 1));
          ra[r] = (m0 + ma < M && k0 + ka < K) ? A[(size_t)(m0 + ma) * sam + (size_t)(k0 + ka) * sak] : 0.0f;
          rb[r] = (n0 + nb < N && k0 + kb < K) ? Bm[(size_t)(n0 + nb) * sbn + (size_t)(k0 + kb) * sbk] : 0.0f;
        }
      };
      fetch(0);
      for (int k0 = 0; k0 < K; k0 += FK) {
        __syncthreads();  // the previous chunk has been read
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int e = t + r * NT;
          const int ka = akc ? (e & (FK - 1)) : (e >> 6), ma = akc ? (e >> 4) : (e & (FT - 1));
          const int kb = bkc ? (e & (FK - 1)) : (e >> 6), nb = bkc ? (e >> 4) : (e & (FT - 1));
          s.a[ka][ma] = ra[r];
          s.b[kb][nb] = rb[r];
        }
        __syncthreads();
        if (k0 + FK < K) fetch(k0 + FK);
#pragma unroll
        for (int kk = 0; kk < FK; ++kk) {
          const float4 av = *reinterpret_cast<const float4*>(&s.a[kk][ty * 4]);
          const float4 bv = *reinterpret_cast<const float4*>(&s.b[kk][tx * 4]);
          const float a4[4] = {av.x, av.y, av.z, av.w}, b4[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a4[i], b4[j], acc[i][j]);
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int m = m0 + ty * 4 + i, n = n0 + tx * 4 + j;
          if (m < M && n < N) epi(m, n, acc[i][j]);
        }
    }
  __syncthreads();  // what the epilogue stored is visible to the whole workgroup
}

// out[n] = sum_m src[m * N + n], m ascending: the two bias gradients
__device__ __forceinline__ void column_sums(const float* src, int M, int N, float* out) {
  for (int n = threadIdx.x; n < N; n += NT) {
    float a = 0.0f;
    for (int m = 0; m < M; ++m) a += src[(size_t)m * N + n];
    out[n] = a;
  }
}

__host__ __device__ inline size_t adv_head_ws_floats(int B, int D, int C, bool term) {
  const size_t H = (size_t)D / 2;
  return 2 * (size_t)B * H + (size_t)B * C + (term ? (size_t)B * D : 0);
}

__global__ __launch_bounds__(NT) void adv_heads_kernel(const AirAdvHeads d) {
  __shared__ FusedLds lds;
  __shared__ double sh[NT / 64];
  __shared__ int shc[NT / 64];
  const int k = blockIdx.x;
  const AirAdvHead& hd = d.head[k];
  const int B = d.B, D = d.D, H = D / 2, C = hd.C;
  const bool term = d.want_dx && d.nheads > 1;
  float* ws = reinterpret_cast<float*>(d.ws);
  for (int q = 0; q < k; ++q) ws += adv_head_ws_floats(B, D, d.head[q].C, term);
  float* hbuf = ws;                          // (B, H) h
  float* kbuf = hbuf + (size_t)B * H;        // (B, H) keep where h > 0, else 0; then d loss / d(w1 x + b1)
  float* obuf = kbuf + (size_t)B * H;        // (B, C) o; then d loss / d(w2 h + b2)
  float* tbuf = obuf + (size_t)B * C;        // (B, D) this head's dx term (several heads)
  float* dw1 = hd.grads;
  float* db1 = dw1 + (size_t)H * D;
  float* dw2 = db1 + H;
  float* db2 = dw2 + (size_t)C * H;
  const float* x = d.feats;

  // the dropout draw of air_dropout_mask_ctr, quad by quad, into kbuf
  const float* keep = hd.keep;
  const bool draw = !keep && hd.p > 0.0f && hd.counter;
  const size_t nmask = (size_t)B * H, quads = (nmask + 3) / 4;
  if (draw) {
    const uint64_t off = *reinterpret_cast<const unsigned long long*>(hd.counter);
    for (size_t q = threadIdx.x; q < quads; q += NT) dropout_quad(kbuf, nmask, hd.p, hd.seed, off, q);
    keep = kbuf;
    __syncthreads();  // every thread has read the counter and the mask is written
    if (threadIdx.x == 0) *reinterpret_cast<unsigned long long*>(hd.counter) = off + quads;
  }

  // h = relu(keep * (w1 x + b1))
  tile_gemm(lds, x, D, 1, hd.w1, D, 1, B, H, D, [&](int b, int j, float v) {
    const size_t e = (size_t)b * H + j;
    const float pre = v + hd.b1[j];
    const float kv = keep ? keep[e] : 1.0f;
    const float h = fmaxf(keep ? pre * kv : pre, 0.0f);
    hbuf[e] = h;
    kbuf[e] = h > 0.0f ? kv : 0.0f;
  });
  // o = relu(w2 h + b2)
  tile_gemm(lds, hbuf, H, 1, hd.w2, H, 1, B, C, H,
            [&](int b, int c, float v) { obuf[(size_t)b * C + c] = fmaxf(v + hd.b2[c], 0.0f); });

  // softmax + CE + accuracy, row per thread: the arithmetic of softmax_ce_fwd_kernel / softmax_ce_bwd_kernel
  {
    double acc = 0.0;
    int hit = 0;
    const float g = 1.0f / (float)B;
    for (int b = threadIdx.x; b < B; b += NT) {
      float* row = obuf + (size_t)b * C;
      float m = row[0];
      int am = 0;
      for (int c = 1; c < C; ++c)
        if (row[c] > m) { m = row[c]; am = c; }
      double sd = 0.0;
      for (int c = 0; c < C; ++c) sd += (double)expf(row[c] - m);
      const float s = (float)sd;
      const float inv = (float)(1.0 / sd);
      const int lab = (int)hd.targets[b];
      if (lab >= 0 && lab < C) acc += (double)(logf(s) - (row[lab] - m));
      hit += am == lab;
      for (int c = 0; c < C; ++c) {
        const float o = row[c];
        const float pr = expf(o - m) * inv;
        row[c] = o > 0.0f ? g * (pr - (c == lab ? 1.0f : 0.0f)) : 0.0f;  // through the ReLU
      }
    }
    acc = air_wave_sum_d(acc);
    for (int o = 32; o > 0; o >>= 1) hit += __shfl_xor(hit, o, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { sh[wave] = acc; shc[wave] = hit; }
    __syncthreads();
    if (threadIdx.x == 0) {
      double t = 0.0;
      int h = 0;
      for (int w = 0; w < NT / 64; ++w) { t += sh[w]; h += shc[w]; }
      *hd.loss = (float)(t / B);
      *hd.correct = h;
      if (hd.run_correct) *hd.run_correct += h;
    }
  }

  // second layer: db2, dw2 = do^T h, dh = do w2, through Dropout -> ReLU
  column_sums(obuf, B, C, db2);
  tile_gemm(lds, obuf, 1, C, hbuf, 1, H, C, H, B, [&](int c, int j, float v) { dw2[(size_t)c * H + j] = v; });
  tile_gemm(lds, obuf, C, 1, hd.w2, 1, H, B, H, C, [&](int b, int j, float v) {
    const size_t e = (size_t)b * H + j;
    kbuf[e] = v * kbuf[e];
  });
  // first layer: db1, dw1 = dh^T x
  column_sums(kbuf, B, H, db1);
  tile_gemm(lds, kbuf, 1, H, x, 1, D, H, D, B, [&](int j, int i, float v) { dw1[(size_t)j * D + i] = v; });
  // gradient reversal (model.py:990-995): this head's term of dx
  if (d.want_dx) {
    float* out = term ? tbuf : d.dx;
    const float nl = -d.lambda;
    tile_gemm(lds, kbuf, H, 1, hd.w1, 1, D, B, D, H, [&](int b, int i, float v) { out[(size_t)b * D + i] = nl * v; });
  }
}

// dx = ((t_0 + t_1) + t_2) + t_3: the heads' terms in head order
__global__ __launch_bounds__(NT) void adv_heads_dx_kernel(const AirAdvHeads d) {
  const size_t n = (size_t)d.B * d.D;
  const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  const float* ws = reinterpret_cast<const float*>(d.ws);
  float a = 0.0f;
  for (int k = 0; k < d.nheads; ++k) {
    const size_t hf = adv_head_ws_floats(d.B, d.D, d.head[k].C, true);
    const float v = ws[hf - n + i];
    a = k == 0 ? v : a + v;
    ws += hf;
  }
  d.dx[i] = a;
}

inline unsigned nblk(size_t n) { return (unsigned)((n + NT - 1) / NT); }

}  // namespace

extern "C" {

int air_dropout_mask(float* keep, size_t n, float p, uint64_t seed, uint64_t offset, air_stream_t stream) {
  if (!keep || n == 0 || !(p >= 0.0f) || !(p < 1.0f)) return AIR_EINVAL;
  hipLaunchKernelGGL(dropout_mask_kernel, dim3(nblk((n + 3) / 4)), dim3(NT), 0, air_stream(stream), keep, n, p, seed,
                     offset);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

int air_dropout_mask_ctr(float* keep, size_t n, float p, uint64_t seed, uint64_t* counter, air_stream_t stream) {
  if (!keep || n == 0 || !(p >= 0.0f) || !(p < 1.0f) || !counter || (reinterpret_cast<size_t>(counter) & 7))
    return AIR_EINVAL;
  const size_t quads = (n + 3) / 4;
  hipLaunchKernelGGL(dropout_mask_ctr_kernel, dim3(nblk(quads)), dim3(NT), 0, air_stream(stream), keep, n, p, seed,
                     reinterpret_cast<const unsigned long long*>(counter));
  AIR_CHECK_LAUNCH();
  hipLaunchKernelGGL(dropout_ctr_add_kernel, dim3(1), dim3(1), 0, air_stream(stream),
                     reinterpret_cast<unsigned long long*>(counter), (unsigned long long)quads);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

int air_mask_relu_fwd(const float* x, const float* keep, size_t n, float* y, air_stream_t stream) {
  if (!x || !y || n == 0) return AIR_EINVAL;
  hipLaunchKernelGGL(mask_relu_fwd_kernel, dim3(nblk(n)), dim3(NT), 0, air_stream(stream), x, keep, n, y);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

int air_mask_relu_bwd(const float* dy, const float* y, const float* keep, size_t n, float alpha, float* dx,
                      air_stream_t stream) {
  if (!dy || !y || !dx || n == 0) return AIR_EINVAL;
  hipLaunchKernelGGL(mask_relu_bwd_kernel, dim3(nblk(n)), dim3(NT), 0, air_stream(stream), dy, y, keep, n, alpha, dx);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

int air_scale(float* x, size_t n, float alpha, air_stream_t stream) {
  if (!x || n == 0) return AIR_EINVAL;
  hipLaunchKernelGGL(scale_kernel, dim3(nblk(n)), dim3(NT), 0, air_stream(stream), x, n, alpha);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

int air_softmax_ce_fwd(const float* logits, const long long* labels, int B, int C, float* probs, float* loss,
                       int* correct_or_null, air_stream_t stream) {
  if (!logits || !labels || !probs || !loss || B <= 0 || C <= 0) return AIR_EINVAL;
  hipLaunchKernelGGL(softmax_ce_fwd_kernel, dim3(1), dim3(NT), 0, air_stream(stream), logits, labels, B, C, probs, loss,
                     correct_or_null);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

int air_softmax_ce_bwd(const float* probs, const long long* labels, int B, int C, const float* gscale_or_null,
                       float* dlogits, air_stream_t stream) {
  if (!probs || !labels || !dlogits || B <= 0 || C <= 0) return AIR_EINVAL;
  hipLaunchKernelGGL(softmax_ce_bwd_kernel, dim3(nblk((size_t)B * C)), dim3(NT), 0, air_stream(stream), probs, labels,
                     B, C, gscale_or_null, dlogits);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

static bool adv_shape_ok(int B, int D, int nheads) {
  return B >= 1 && B <= 4096 && D >= 2 && D <= 1024 && (D & 1) == 0 && nheads >= 1 && nheads <= AIR_ADV_MAX_HEADS;
}

size_t air_adv_heads_ws_bytes(int B, int D, int nheads, const int* C, int want_dx) {
  if (!adv_shape_ok(B, D, nheads) || !C) return 0;
  size_t n = 0;
  for (int k = 0; k < nheads; ++k) {
    if (C[k] < 1 || C[k] > 256) return 0;
    n += adv_head_ws_floats(B, D, C[k], want_dx && nheads > 1);
  }
  return n * sizeof(float);
}

int air_adv_heads(const AirAdvHeads* d, air_stream_t stream) {
  if (!d || !adv_shape_ok(d->B, d->D, d->nheads) || !d->feats || !d->ws || (d->want_dx && !d->dx) ||
      !(d->lambda == d->lambda))
    return AIR_EINVAL;
  size_t need = 0;
  for (int k = 0; k < d->nheads; ++k) {
    const AirAdvHead& h = d->head[k];
    if (!h.w1 || !h.b1 || !h.w2 || !h.b2 || !h.targets || !h.grads || !h.loss || !h.correct) return AIR_EINVAL;
    if (h.C < 1 || h.C > 256 || !(h.p >= 0.0f) || !(h.p < 1.0f)) return AIR_EINVAL;
    if (h.counter) {
      if (reinterpret_cast<size_t>(h.counter) & 7) return AIR_EINVAL;
      for (int q = 0; q < k; ++q)  // each workgroup advances its own counter
        if (d->head[q].counter == h.counter) return AIR_EINVAL;
    }
    need += adv_head_ws_floats(d->B, d->D, h.C, d->want_dx && d->nheads > 1) * sizeof(float);
  }
  if (d->ws_bytes < need || (reinterpret_cast<size_t>(d->ws) & 15)) return AIR_EINVAL;
  hipLaunchKernelGGL(adv_heads_kernel, dim3(d->nheads), dim3(NT), 0, air_stream(stream), *d);
  AIR_CHECK_LAUNCH();
  if (d->want_dx && d->nheads > 1) {
    hipLaunchKernelGGL(adv_heads_dx_kernel, dim3(nblk((size_t)d->B * d->D)), dim3(NT), 0, air_stream(stream), *d);
    AIR_CHECK_LAUNCH();
  }
  return AIR_OK;
}

}  // extern "C"
