// What every kernel on the ragged PCM path (rows of Lcap samples, fp32 or 16-bit, the row's own length in device
// memory) reads its input through.
#pragma once
#include <hip/hip_runtime.h>

// sample i (an int or a long) as the float the reference's loader hands on: fp32 as it is, 16-bit PCM as s / 32768 (exact)
template <typename I>
__device__ __forceinline__ float air_pcm_sample(const float* __restrict__ p, I i) { return p[i]; }
template <typename I>
__device__ __forceinline__ float air_pcm_sample(const short* __restrict__ p, I i) { return (float)p[i] * (1.0f / 32768.0f); }

// samples of row b: its length from device memory, kept inside the row (ragged), or the whole row (lengths NULL)
__device__ __forceinline__ int air_row_len(const int* __restrict__ lengths, int b, int Lcap) {
  return lengths ? min(max(lengths[b], 1), Lcap) : Lcap;
}

__device__ __forceinline__ void atomic_max_pos(unsigned* p, float v) {
  atomicMax(p, __float_as_uint(v));  // v >= 0: unsigned order == float order
}
