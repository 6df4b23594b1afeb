// Philox4x32-10 and what the kernels derive from it - the one device-side statement; tests/philox_oracle.py is the
// host-side one.  A block is addressed by a 64-bit counter and a 64-bit key: counter words {ctr lo, ctr hi, 0, 0},
// key words {key lo, key hi}.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

__device__ __forceinline__ void air_philox_rounds(uint32_t (&c)[4], uint64_t key) {
  uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
    const uint32_t n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    const uint32_t n3 = (uint32_t)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

__device__ __forceinline__ void air_philox_block(uint64_t ctr, uint64_t key, uint32_t (&c)[4]) {
  c[0] = (uint32_t)ctr; c[1] = (uint32_t)(ctr >> 32); c[2] = 0u; c[3] = 0u;
  air_philox_rounds(c, key);
}

constexpr float AIR_PHILOX_INV = 2.3283064365386963e-10f;  // 2^-32

// a word as a uniform in [0, 1): one fp32 rounding of w and an exact scaling
__device__ __forceinline__ float air_philox_u01(uint32_t w) { return (float)w * AIR_PHILOX_INV; }

// four standard normals of one block: Box-Muller on the word pairs (0, 1) and (2, 3), u1 in (0, 1]
__device__ __forceinline__ void air_philox_randn_quad(const uint32_t (&c)[4], float (&z)[4]) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float u1 = ((float)c[2 * h] + 1.0f) * AIR_PHILOX_INV;  // (0, 1]
    const float u2 = air_philox_u01(c[2 * h + 1]);
    const float r = sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincosf(6.283185307179586f * u2, &sn, &cs);
    z[2 * h] = r * cs;
    z[2 * h + 1] = r * sn;
  }
}
