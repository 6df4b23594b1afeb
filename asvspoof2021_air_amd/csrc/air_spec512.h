// The 512-point power-spectrum pipeline of the PCM front-ends, stated once: LFCC (csrc/lfcc.hip), STFT and Melspec
// (csrc/spectral.hip).  All three give 16 lanes to a frame and 4 frames to a wave, stage a tile of PCM in LDS, run the
// 512-point real FFT as a 256-point complex FFT on the even/odd packing - 16 x 16 with the radix-16 butterfly of
// air_fft16.h, transposed through a padded wave-private LDS tile - and untangle it against lane (16 - g) of the same
// 16-lane group.  What differs between the kernels is a template parameter, never a run-time flag: the hop, the staged
// span (NSAMP) and its first sample, the reflect branch (Melspec), the frames a tile writes (FW; LFCC computes a halo
// beside them) and the silence frame (LFCC).  The bits of these kernels are pinned to the reference: a change here
// changes all of them, and tests/test_spectral_gpu.py holds LFCC and STFT to one spectrum.
//
// What stays with the kernels, and why.  The window multiply, the first fft16 and the w256 twiddle multiply: LFCC
// holds the window and w256^(g q) in registers across its barrier, spec_kernel reads them from the plan at use.  The
// loop over a lane's 16 bins and the store of each power value (spec512_bin_power gives the value): with the loop in
// here hipcc schedules lfcc_kernel on 123 VGPRs for 89, 27.5 us for 26.7 at B = 64 x 4 s.  LFCC's staging loop:
// lfcc.hip states spec512_stage again, 26.9 us for 26.7 through the helper (profiles/spectral_frontends.md).
#pragma once
#include <math.h>

#include "air_common.h"
#include "air_fft16.h"
#include "air_pcm.h"

namespace {

constexpr int SPEC512_XROW = 17;  // padded transpose row (complex elements): conflict-free both ways

// (cos, sin)(2 pi 16 p / 512), p = 0 .. 15: bin g + 16 p turns the lane's (cos, sin)(2 pi g / 512) by these
__device__ __constant__ const float W32C[16] = {
    1.000000000f, 0.980785280f, 0.923879533f, 0.831469612f, 0.707106781f, 0.555570233f,
    0.382683432f, 0.195090322f, 0.000000000f, -0.195090322f, -0.382683432f, -0.555570233f,
    -0.707106781f, -0.831469612f, -0.923879533f, -0.980785280f};
__device__ __constant__ const float W32S[16] = {
    0.000000000f, 0.195090322f, 0.382683432f, 0.555570233f, 0.707106781f, 0.831469612f,
    0.923879533f, 0.980785280f, 1.000000000f, 0.980785280f, 0.923879533f, 0.831469612f,
    0.707106781f, 0.555570233f, 0.382683432f, 0.195090322f};

// ---- host: the tables of a plan ------------------------------------------------
constexpr double SPEC512_PI = 3.14159265358979323846;

// tw256[2 n] = e^{-2 pi i n/256}: (re, im), n = 0..255;  tw512[2 q] = e^{-2 pi i q/512}, q = 0..15
inline void spec512_fill_twiddles(float* tw256, float* tw512) {
  for (int n = 0; n < 256; ++n) {
    tw256[2 * n] = (float)cos(2.0 * SPEC512_PI * n / 256.0);
    tw256[2 * n + 1] = (float)(-sin(2.0 * SPEC512_PI * n / 256.0));
  }
  for (int q = 0; q < 16; ++q) {
    tw512[2 * q] = (float)cos(2.0 * SPEC512_PI * q / 512.0);
    tw512[2 * q + 1] = (float)(-sin(2.0 * SPEC512_PI * q / 512.0));
  }
}

// periodic Hamming window (torch.hamming_window): LFCC's default window and the STFT window
inline void spec512_fill_hamming(float* w, int n_taps) {
  for (int n = 0; n < n_taps; ++n) w[n] = (float)(0.54 - 0.46 * cos(2.0 * SPEC512_PI * n / n_taps));
}

// ---- ragged row geometry -------------------------------------------------------
struct Spec512Row {
  int L, T;        // samples and frames of this row
  int live_tiles;  // tiles of the row that write frames: they share the row's constant frames
  bool dead;       // this tile holds no frame that the row writes (workgroup-uniform)
};

// Row b of a ragged batch: its length from device memory, its frames at hop HOP, and whether the tile that writes
// frames [t0, t0 + FW) has anything to write.  OPTIONAL: lengths may be null (every row holds Lcap samples).
template <int HOP, int FW, bool OPTIONAL>
__device__ __forceinline__ Spec512Row spec512_row(const int* __restrict__ lengths, const int* __restrict__ start, int b,
                                                  int Lcap, int feat_len, int t0) {
  Spec512Row r;
  r.L = Lcap;
  if (!OPTIONAL || lengths != nullptr) r.L = min(max(lengths[b], 1), Lcap);  // a bad length must not read outside the row
  r.T = 1 + r.L / HOP;
  r.live_tiles = (r.T + FW - 1) / FW;
  r.dead = t0 >= r.T;
  if (r.T > feat_len) {
    // chopped row: only the tiles that overlap [start, start + feat_len) are written (same clamp as spec512_store_padded)
    const int st = start != nullptr ? min(max(start[b], 0), r.T - feat_len) : 0;
    r.dead = r.dead || t0 + FW <= st || t0 >= st + feat_len;
  }
  return r;
}

// ---- PCM tile staging ----------------------------------------------------------
// s_pcm[e] = sample s0 + e of the row (s0 may be < 0, a multiple of 4), e < NSAMP, zero outside [0, L); pre-emphasised
// when emph: the non-recursive FIR on the ORIGINAL samples, two roundings like the reference.  Rows are fp32 (row) or
// 16-bit PCM (row16 non-null).  MAY_REFLECT (Melspec): with reflect, numpy's "reflect" instead of zeros - x[-m] in
// front, x[2 (L - 1) - m] behind; one reflection, then clamped into the row - what a frame of a row of at least 257
// samples reads is never clamped, and nothing can read outside a shorter one.  (spec_kernel's; lfcc_body states the
// MAY_REFLECT = false form itself, see above.)
template <int NSAMP, int NT, bool MAY_REFLECT>
__device__ __forceinline__ void spec512_stage(const float* __restrict__ row, const short* __restrict__ row16, int L,
                                              long s0, bool emph, bool reflect, float* __restrict__ s_pcm, int tid) {
  // sample m of this utterance as the float the reference's loader hands to the front-end
  auto sample = [&](long m) -> float { return row16 ? air_pcm_sample(row16, m) : row[m]; };
  const bool vec_ok = row16 == nullptr && ((((size_t)row) & 15) == 0);
  for (int e4 = tid; e4 < NSAMP / 4; e4 += NT) {
    const long n = s0 + 4 * (long)e4;
    float v[4];
    if (vec_ok && n >= 0 && n + 3 < L) {
      const float4 q = *reinterpret_cast<const float4*>(row + n);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
      if (emph) {
        const float prev = n > 0 ? row[n - 1] : 0.0f;
        v[3] = __fsub_rn(v[3], __fmul_rn(0.97f, v[2]));
        v[2] = __fsub_rn(v[2], __fmul_rn(0.97f, v[1]));
        v[1] = __fsub_rn(v[1], __fmul_rn(0.97f, v[0]));
        if (n > 0) v[0] = __fsub_rn(v[0], __fmul_rn(0.97f, prev));
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        long m = n + k;
        float x = 0.0f;
        if (MAY_REFLECT && reflect) {
          if (m < 0) m = -m;
          else if (m >= L) m = 2 * ((long)L - 1) - m;
          m = m < 0 ? 0 : (m > L - 1 ? L - 1 : m);
          x = sample(m);
        } else if (m >= 0 && m < L) {
          x = sample(m);
          if (emph && m > 0) x = __fsub_rn(x, __fmul_rn(0.97f, sample(m - 1)));
        }
        v[k] = x;
      }
    }
    *reinterpret_cast<float4*>(&s_pcm[4 * e4]) = make_float4(v[0], v[1], v[2], v[3]);
  }
}

// ---- per-lane constants of the untangle ----------------------------------------
struct Spec512Lane {
  float cq, sq;  // (cos, sin)(2 pi g/512), g = lane & 15
  int partner;   // lane (16 - g) & 15 of the same 16-lane group
};
__device__ __forceinline__ Spec512Lane spec512_lane(const float* __restrict__ tw512, int lane) {
  const int g = lane & 15;
  return Spec512Lane{tw512[2 * g], -tw512[2 * g + 1], (lane & 48) | ((16 - g) & 15)};
}

// ---- second half of the 256-point FFT ------------------------------------------
// In: x[q] = Y[g][q] w256^(g q) of frame f (the first fft16 and the twiddle multiply are the caller's).  The 16 x 16
// transpose goes through the wave-private tile xch (4 x 16 x SPEC512_XROW floats) - row q, column g; real parts, then
// imaginary parts through the same 4.3 KB - and a second fft16 over l finishes it.  Out: x[p] = Z[g + 16 p]; xch is
// free for the caller again.
__device__ __forceinline__ void spec512_transpose_fft(cf (&x)[16], float* xch, int f, int g) {
  float xre[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) xch[(f * 16 + q) * SPEC512_XROW + g] = x[q].x;
  air_wave_lds_fence();
#pragma unroll
  for (int l = 0; l < 16; ++l) xre[l] = xch[(f * 16 + g) * SPEC512_XROW + l];
  air_wave_lds_fence();
#pragma unroll
  for (int q = 0; q < 16; ++q) xch[(f * 16 + q) * SPEC512_XROW + g] = x[q].y;
  air_wave_lds_fence();
#pragma unroll
  for (int l = 0; l < 16; ++l) x[l] = cf{xre[l], xch[(f * 16 + g) * SPEC512_XROW + l]};
  fft16<false>(x);
  air_wave_lds_fence();
}

// ---- real-FFT untangle + power -------------------------------------------------
// In: x[p] = Z[g + 16 p].  Out: |X_k|^2 of this lane's bin k = g + 16 p, which pairs with 256 - k: lane (16-g)&15, index
// 15-p (g != 0); own lane, index (16-p)&15 (g == 0).  The reference takes norm(., 2, -1).pow(2), i.e.
// fl(fl(sqrt(s))^2) - within 1.5 ulp of s itself; the power is taken directly (X holds 2 x the bin: the factor 0.25 is
// exact).  Called for p = 0 .. 15 from a fully unrolled loop: x lives in registers.
__device__ __forceinline__ float spec512_bin_power(const cf (&x)[16], int p, int g, Spec512Lane ln) {
  const int pp = 15 - p;
  float bre = __shfl(x[pp].x, ln.partner, 64);
  float bim = __shfl(x[pp].y, ln.partner, 64);
  const int p0 = (16 - p) & 15;
  if (g == 0) {
    bre = x[p0].x;
    bim = x[p0].y;
  }
  // E2 = A + conj(B), O2 = A - conj(B);  2X = E2 - i w512^k O2 - on register pairs (same roundings as the scalar
  // form: xr = (ere + c oim) - s ore, xi = (eim - c ore) - s oim)
  const cf A = x[p], Bv = cf{bre, bim};
  const cf E = __builtin_elementwise_fma(Bv, cf{1.0f, -1.0f}, A);  // (A.re + bre, A.im - bim)
  const cf O = __builtin_elementwise_fma(Bv, cf{-1.0f, 1.0f}, A);  // (A.re - bre, A.im + bim)
  const cf cs = cmul(cf{ln.cq, ln.sq}, cf{W32C[p], W32S[p]});  // (cos, sin)(2 pi k / 512)
  const cf P1 = LFCC_LO(cs) * LFCC_SWAP(O);                    // (c oim, c ore)
  const cf X1 = __builtin_elementwise_fma(P1, cf{1.0f, -1.0f}, E);
  const cf X = X1 - LFCC_HI(cs) * O;                           // - (s ore, s oim)
  const cf X2 = X * X;
  return 0.25f * (X2.x + X2.y);
}
// |X_256|^2, held by lane g == 0:  X[256] = Re Z0 - Im Z0 (real)
__device__ __forceinline__ float spec512_nyquist_power(const cf (&x)[16]) {
  const float ny = x[0].x - x[0].y;
  return ny * ny;
}

// ---- stores --------------------------------------------------------------------
// (B, T, D): the tile s_out[fo][D] is the output's own layout, n = frames x D floats from orow on
template <int NT>
__device__ __forceinline__ void spec512_store_dense(float* __restrict__ orow, const float* __restrict__ s_out, int n,
                                                    int D, int tid) {
  if ((D & 3) == 0 && ((reinterpret_cast<size_t>(orow) & 15) == 0)) {
    for (int e = tid; e < n / 4; e += NT)
      reinterpret_cast<float4*>(orow)[e] = reinterpret_cast<const float4*>(s_out)[e];
  } else {
    for (int e = tid; e < n; e += NT) orow[e] = s_out[e];
  }
}

// (B, D, feat_len) from the tile s_out[c][FW + 1] (odd stride: conflict-free along the frames), obase = row b of out:
// frame t of T lands on t' = t - start (T >= feat_len: the crop, start clamped so that no column stays unwritten), on
// every t + k T (AIR_PAD_REPEAT), or on t behind / in front of the feat_len - T constant frames (dataset.py:72-79):
// zeros appended (:513-517) or, SILENCE (LFCC only), the D-float silence frame PREPENDED (:524-528).  The constant
// frames are shared out over the row's live tiles.
template <int FW, int NT, bool SILENCE>
__device__ __forceinline__ void spec512_store_padded(float* __restrict__ obase, const float* __restrict__ s_out, int D,
                                                     int T, int t0, int tile, int live_tiles, int flen,
                                                     const int* __restrict__ start_dev, int b, int pad_mode,
                                                     const float* __restrict__ silence, int tid) {
  constexpr int OSTR = FW + 1;
  const int start = (start_dev != nullptr && T > flen) ? min(max(start_dev[b], 0), T - flen) : 0;
  const int npad = flen - T;  // > 0: pad
  const int shift = (SILENCE && npad > 0 && pad_mode == AIR_PAD_SILENCE) ? npad : 0;
  for (int e = tid; e < FW * D; e += NT) {
    const int c = e / FW, fo = e - c * FW;
    const int t = t0 + fo;
    if (t >= T) continue;
    const float v = s_out[c * OSTR + fo];
    if (T >= flen) {
      const int tp = t - start;
      if (tp >= 0 && tp < flen) obase[(size_t)c * flen + tp] = v;
    } else if (pad_mode == AIR_PAD_REPEAT) {
      for (int tp = t; tp < flen; tp += T) obase[(size_t)c * flen + tp] = v;
    } else {
      obase[(size_t)c * flen + t + shift] = v;
    }
  }
  if (npad > 0 && (SILENCE ? pad_mode != AIR_PAD_REPEAT : pad_mode == AIR_PAD_ZERO)) {
    const int lo = (SILENCE && pad_mode == AIR_PAD_SILENCE) ? 0 : T;
    for (int e = tile * NT + tid; e < npad * D; e += live_tiles * NT) {
      const int c = e / npad, k = e - c * npad;
      obase[(size_t)c * flen + lo + k] = (SILENCE && pad_mode == AIR_PAD_SILENCE) ? silence[c] : 0.0f;
    }
  }
}

}  // namespace
