// Fusion of the scores of K systems (score_fusion.py:21-43 of the reference): per trial the sum (avg_fuse) or the mean
// over the systems that have it (weighted_fuse) of the - optionally weighted - fp32 scores, with the arithmetic pandas'
// group sum / group mean perform on a float32 column: a compensated (Kahan) fp32 accumulation in file order k = 0 .. K-1,
// the weight product rounded to fp32 on its own first, NaN scores skipped and not counted, a compensation that turned NaN
// (an infinite score) reset to zero, the mean one correctly rounded fp32 division by the count.  tests/fusion_oracle.py
// states the same in numpy; tests/golden/fusion.npz holds pandas' bits.
//
// One thread per trial.  Aligned path (index NULL): thread n reads scores[k * row_stride + n], K coalesced row reads.
// Indexed path: thread n reads the K positions index[k * N + n] (coalesced) and gathers the scores - the outer join of
// K score files in their own row orders without materialising the aligned matrix.  (K + 1) * 4 * N bytes of traffic
// (twice that with an index): nothing to tune.
//
// Every operation is a single correctly rounded fp32 instruction (__fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn): no
// contraction can fuse the weight product into the compensation.
#include "air_common.h"

#include <cmath>

namespace {

constexpr int kFuseThreads = 256;
constexpr int kFuseMaxSystems = 64;

template <bool INDEXED, bool WEIGHTED>
__global__ __launch_bounds__(kFuseThreads) void score_fuse_kernel(const float* __restrict__ scores, int64_t row_stride,
                                                                  const int32_t* __restrict__ index,
                                                                  const float* __restrict__ weights, int K, int64_t N,
                                                                  int mode, float* __restrict__ out,
                                                                  uint32_t* __restrict__ n_present) {
  const int64_t n = (int64_t)blockIdx.x * kFuseThreads + threadIdx.x;
  if (n >= N) return;
  float acc = 0.0f, comp = 0.0f;
  uint32_t count = 0;
  for (int k = 0; k < K; ++k) {
    int64_t pos = n;
    if (INDEXED) {
      const int32_t q = index[(int64_t)k * N + n];
      if (q < 0 || (int64_t)q >= row_stride) continue;  // absent (or outside the row: never dereferenced)
      pos = q;
    }
    float v = scores[(int64_t)k * row_stride + pos];
    if (WEIGHTED) v = __fmul_rn(v, weights[k]);
    if (v != v) continue;  // pandas skips NaN and does not count it
    const float y = __fsub_rn(v, comp);
    const float t = __fadd_rn(acc, y);
    const float c = __fsub_rn(__fsub_rn(t, acc), y);
    comp = (c != c) ? 0.0f : c;  // an infinite term: the sum stays +-inf instead of turning NaN
    acc = t;
    ++count;
  }
  float r = mode ? __fdiv_rn(acc, (float)count) : acc;
  if (count == 0) r = __builtin_nanf("");
  out[n] = r;
  if (n_present) n_present[n] = count;
}

}  // namespace

extern "C" {

int air_score_fuse_max_systems(void) { return kFuseMaxSystems; }

int air_score_fuse(const float* scores, int64_t row_stride, const int32_t* index, const float* weights, int K, int64_t N,
                   int mode, float* out, uint32_t* n_present, air_stream_t stream) {
  if (K < 1 || N < 0 || (mode != 0 && mode != 1)) return AIR_EINVAL;
  if (K > kFuseMaxSystems) return AIR_EUNSUPPORTED;
  if (N == 0) return AIR_OK;
  if (!scores || !out) return AIR_EINVAL;
  const int64_t row = index ? row_stride : N;  // floats of a row that may be read
  if (row < 1 || (K > 1 && row_stride < row)) return AIR_EINVAL;
  if (N > ((int64_t)1 << 38) || row_stride > ((int64_t)1 << 38)) return AIR_EUNSUPPORTED;
  const float* lo = scores;
  const float* hi = scores + (int64_t)(K - 1) * row_stride + row;
  if (out < hi && out + N > lo) return AIR_EINVAL;  // out overlaps scores
  const dim3 grid((unsigned)((N + kFuseThreads - 1) / kFuseThreads)), block(kFuseThreads);
  hipStream_t st = air_stream(stream);
#define AIR_FUSE_LAUNCH(I, W) \
  hipLaunchKernelGGL((score_fuse_kernel<I, W>), grid, block, 0, st, scores, row_stride, index, weights, K, N, mode, out, n_present)
  if (index) {
    if (weights) AIR_FUSE_LAUNCH(true, true); else AIR_FUSE_LAUNCH(true, false);
  } else {
    if (weights) AIR_FUSE_LAUNCH(false, true); else AIR_FUSE_LAUNCH(false, false);
  }
#undef AIR_FUSE_LAUNCH
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

}  // extern "C"
