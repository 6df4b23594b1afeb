// ITU-T G.711 in plain integer arithmetic, as CPython's audioop states it (lin2ulaw / ulaw2lin / lin2alaw / alaw2lin at
// width 2): mu-law codes the top 14 bits of a 16-bit sample, A-law the top 13.  Host and device: tests/test_codec_gpu.py
// holds the device side to audioop on all 65 536 inputs.
#pragma once
#include <hip/hip_runtime.h>

// floor(log2(v)), v >= 1
__host__ __device__ __forceinline__ int g711_log2(int v) { return 31 - __builtin_clz((unsigned)v); }

// s in [-32768, 32767] -> 8-bit mu-law code
__host__ __device__ __forceinline__ int g711_ulaw_encode(int s) {
  int v = s >> 2, mask = 0xFF;  // (arithmetic shift)
  if (v < 0) {
    v = 0x21 - v;
    mask = 0x7F;
  } else {
    v += 0x21;
  }
  if (v > 8159) v = 8159;
  const int seg = g711_log2(v) - 5;  // 33 <= v <= 8159: segment 0 .. 7
  return ((seg << 4) | ((v >> (seg + 1)) & 0xF)) ^ mask;
}

__host__ __device__ __forceinline__ int g711_ulaw_decode(int code) {
  const int u = ~code & 0xFF;
  const int t = (((u & 0xF) << 3) + 0x84) << ((u & 0x70) >> 4);
  return (u & 0x80) ? 0x84 - t : t - 0x84;
}

// s in [-32768, 32767] -> 8-bit A-law code
__host__ __device__ __forceinline__ int g711_alaw_encode(int s) {
  int v = s >> 3, mask = 0xD5;
  if (v < 0) {
    v = -v - 1;
    mask = 0x55;
  }
  const int seg = v < 32 ? 0 : g711_log2(v) - 4;  // v <= 4095: segment 0 .. 7
  return ((seg << 4) | ((v >> (seg < 2 ? 1 : seg)) & 0xF)) ^ mask;
}

__host__ __device__ __forceinline__ int g711_alaw_decode(int code) {
  const int a = code ^ 0x55, seg = (a & 0x70) >> 4;
  int t = (a & 0xF) << 4;
  t = seg == 0 ? t + 8 : (t + 0x108) << (seg - 1);
  return (a & 0x80) ? t : -t;
}

// law 0: mu-law, otherwise A-law
__host__ __device__ __forceinline__ int g711_encode(int law, int s) { return law == 0 ? g711_ulaw_encode(s) : g711_alaw_encode(s); }
__host__ __device__ __forceinline__ int g711_decode(int law, int code) { return law == 0 ? g711_ulaw_decode(code) : g711_alaw_decode(code); }
