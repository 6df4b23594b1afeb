// On-the-fly channel augmentation in the front-end (BASELINE.json configs[4]):
// y_b = (x_b * h_{idx[b]})[:L], optionally rescaled so max|y_b| = max|x_b| ("safe": no clipping, no
// level change).  The reference does this OFFLINE by shelling out to idiap/acoustic-simulator's
// degrade-audio-safe-random.py (channel_simulation/simulated_device.py:33-35,46-50,57-61), a tool
// that is not vendored: PARITY UNPINNED - the arithmetic here follows this repo's own spec
// (oracle/channel.py, checked against scipy.signal.fftconvolve).
//
// Direct time-domain FIR on the fp32 VALU (2*L*H FLOP per utterance: 131 MFLOP at H = 1024 taps;
// HBM traffic is only 2 x 256 KB per utterance, so this is compute-bound, not a byte mover):
//   * a workgroup owns 2048 consecutive outputs of one utterance, a thread 8 consecutive ones;
//   * taps are consumed in chunks of 1024: the x segment a chunk needs (3071 samples) and the
//     tap chunk are staged in LDS once, zero-filled outside [0, L);
//   * per 8 taps a thread holds a 16-sample register window (two aligned groups of 8), does 64
//     FMAs, and slides by ONE new group: 2 ds_read_b128 of x + 2 broadcast ds_read_b128 of taps
//     per 64 FMAs;
//   * LDS layout: every group of 8 samples sits at a 48-byte stride, so the 16 lanes a
//     ds_read_b128 cycle serves (thread t reads group t - jb + const) cover all 64 banks.
//
// Round 5: impulse responses of 128 .. 1025 taps (the bank's 1024) go through OVERLAP-SAVE FFT convolution instead -
// 26 x fewer floating-point operations than the direct form at H = 1024 (the direct kernel runs at 71 % of the fp32
// VALU rate: packed fp32 issues at half rate on this part, there was nothing left in it).  One workgroup transforms TWO
// consecutive 3072-sample output blocks of one utterance at once, as the real and imaginary parts of one 4096-point
// complex FFT (h is real, so Re / Im of the product's inverse are the two blocks' convolutions): 4096 = 16 x 16 x 16,
// three radix-16 passes in registers (air_fft16.h, the LFCC kernel's butterfly) with the data crossing LDS between
// them; the forward transform leaves the spectrum digit-reversed, the IR spectra are stored in the same order and the
// inverse passes run the other way round, so nothing is ever re-ordered; the first pass reads PCM straight from
// global memory and the last one writes y straight to it.  Same result as the direct form to fp32 FFT rounding
// (~3e-7 of the output scale; tests/test_augment.py holds both to the same bound).
//
// Ragged batches (air_ir_convolve_ragged): the same two kernels, templated on the sample type (fp32, or 16-bit PCM
// converted as s / 32768 while it is staged) and given the row capacity Lcap plus the per-row lengths in device memory.
// Row b is convolved, peak-measured and rescaled over its own L_b = clamp(lengths[b], 1, Lcap) samples only: L_b takes
// the place of L in the staging clamp and at the store, nothing inside the FMA / butterfly loops knows about it, so
// y[b, :L_b] carries the bits of the dense call on that utterance alone.  [L_b, Lcap) is written as zero; a workgroup
// whose outputs all lie there stores its zeros and returns.  The dense entry point launches the fp32 instantiation
// without lengths (L_b = Lcap = L).
//
// Banks of responses of different lengths, up to 65 536 taps (air_ir_bank_convolve): rows that drew at most 1025 taps run
// the overlap-save form above, longer ones its uniformly partitioned extension - 4096-point transforms, partitions and
// hop of 2048 samples, the products accumulated in the frequency domain and one inverse per pair of output blocks.  The
// geometry is described in front of those kernels, at the end of the anonymous namespace.
#include "air_common.h"
#include "air_fft16.h"
#include "air_options.h"
#include "air_pcm.h"
#include "g711.h"

namespace {

constexpr int FIR_NT = 256, FIR_R = 8, FIR_BLK = FIR_NT * FIR_R, FIR_KC = 1024;
constexpr int FIR_GROUPS = (FIR_BLK + FIR_KC) / 8;  // 384 groups of 8 samples per staged segment
constexpr int FIR_GS = 12;                           // floats per group slot (8 data + 4 pad)

// y[n0 + i] = x[n0 + i] for n0 + i < L, 0 up to Lcap (i < span): pass-through rows, and with n0 >= L the dead tail
template <typename T>
__device__ __forceinline__ void ir_copy_span(const T* __restrict__ xb, float* __restrict__ yb, int n0, int span, int L, int Lcap,
                                             int t, int nt) {
  for (int n = n0 + t; n < min(n0 + span, Lcap); n += nt) yb[n] = n < L ? air_pcm_sample(xb, n) : 0.0f;
}

template <typename T>
__global__ __launch_bounds__(FIR_NT) void fir_kernel(const T* __restrict__ x, int Lcap, const int* __restrict__ lengths,
                                                     const float* __restrict__ irs, int H,
                                                     const int* __restrict__ idx, float* __restrict__ y,
                                                     unsigned* __restrict__ peaks, int n_ir) {
  __shared__ __attribute__((aligned(16))) float xs[FIR_GROUPS * FIR_GS];
  __shared__ __attribute__((aligned(16))) float hs[FIR_KC];
  const int b = blockIdx.y, n0 = blockIdx.x * FIR_BLK, t = threadIdx.x;
  const int L = air_row_len(lengths, b, Lcap);
  const T* __restrict__ xb = x + (size_t)b * Lcap;
  float* __restrict__ yb = y + (size_t)b * Lcap;
  const int ir = idx ? min(idx[b], n_ir - 1) : 0;  // indices are caller data: never read past the IR table
  if (ir < 0 || n0 >= L) {  // pass-through utterance, or a block wholly behind the row's length: zeros
    ir_copy_span(xb, yb, n0, FIR_BLK, L, Lcap, t, FIR_NT);
    return;
  }
  const float* __restrict__ hb = irs + (size_t)ir * H;
  float out[FIR_R];
#pragma unroll
  for (int r = 0; r < FIR_R; ++r) out[r] = 0.0f;
  float xpeak = 0.0f;

  for (int kc = 0; kc < H; kc += FIR_KC) {
    __syncthreads();
    // staged position p <-> sample m = n0 - kc - (FIR_KC - 1) + p
    const int m0 = n0 - kc - (FIR_KC - 1);
    for (int p = t; p < FIR_GROUPS * 8; p += FIR_NT) {
      const int m = m0 + p;
      const float v = (m >= 0 && m < L) ? air_pcm_sample(xb, m) : 0.0f;
      xs[(p >> 3) * FIR_GS + (p & 7)] = v;
      if (kc == 0 && p >= FIR_KC - 1) xpeak = fmaxf(xpeak, fabsf(v));  // this block's own samples
    }
    for (int j = t; j < FIR_KC; j += FIR_NT) hs[j] = kc + j < H ? hb[kc + j] : 0.0f;
    __syncthreads();
    const int nj = (min(FIR_KC, H - kc) + 7) >> 3;
    // window: whi = group (t + 127 - jb) + 1, wlo = group (t + 127 - jb); see header
    float wlo[8], whi[8];
    {
      const float4* g = reinterpret_cast<const float4*>(xs + (t + 128) * FIR_GS);
      const float4 a = g[0], c = g[1];
      whi[0] = a.x; whi[1] = a.y; whi[2] = a.z; whi[3] = a.w;
      whi[4] = c.x; whi[5] = c.y; whi[6] = c.z; whi[7] = c.w;
    }
    for (int jb = 0; jb < nj; ++jb) {
      const float4* g = reinterpret_cast<const float4*>(xs + (t + 127 - jb) * FIR_GS);
      const float4 a = g[0], c = g[1];
      wlo[0] = a.x; wlo[1] = a.y; wlo[2] = a.z; wlo[3] = a.w;
      wlo[4] = c.x; wlo[5] = c.y; wlo[6] = c.z; wlo[7] = c.w;
      const float4 h0 = reinterpret_cast<const float4*>(hs + jb * 8)[0];
      const float4 h1 = reinterpret_cast<const float4*>(hs + jb * 8)[1];
      const float h[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int r = 0; r < FIR_R; ++r) {
          const int w = r - i + 7;  // 0..14 within [wlo | whi]
          out[r] = fmaf(h[i], w < 8 ? wlo[w] : whi[w - 8], out[r]);
        }
#pragma unroll
      for (int i = 0; i < 8; ++i) whi[i] = wlo[i];
    }
  }
  float ypeak = 0.0f;
#pragma unroll
  for (int r = 0; r < FIR_R; ++r) {
    const int n = n0 + t * FIR_R + r;
    if (n < L) {
      yb[n] = out[r];
      ypeak = fmaxf(ypeak, fabsf(out[r]));
    } else if (n < Lcap) {
      yb[n] = 0.0f;
    }
  }
  if (peaks) {
    xpeak = air_wave_max(xpeak);
    ypeak = air_wave_max(ypeak);
    if ((t & 63) == 0) {
      atomic_max_pos(peaks + 2 * b, xpeak);
      atomic_max_pos(peaks + 2 * b + 1, ypeak);
    }
  }
}

// y_b *= max|x_b| / max|y_b|  (augmented utterances only; the row's own samples only)
__global__ __launch_bounds__(256) void fir_rescale_kernel(float* __restrict__ y, int Lcap, const int* __restrict__ lengths,
                                                          const int* __restrict__ idx, const unsigned* __restrict__ peaks) {
  const int b = blockIdx.y;
  if (idx && idx[b] < 0) return;
  const float px = __uint_as_float(peaks[2 * b]), py = __uint_as_float(peaks[2 * b + 1]);
  if (!(py > 0.0f)) return;
  const float g = px / py;
  const int L = air_row_len(lengths, b, Lcap);
  float* __restrict__ yb = y + (size_t)b * Lcap;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < L; i += gridDim.x * 256) yb[i] *= g;
}

// ---- overlap-save FFT form -------------------------------------------------------------------------------------------
constexpr int FC_N = 4096;            // complex transform length = real block length (two real blocks per transform)
constexpr int FC_V = 3072;            // outputs kept per real block
constexpr int FC_OV = FC_N - FC_V;    // 1024 samples of history in front of a block: taps - 1 <= 1024
constexpr int FC_NT = 256;
constexpr int FC_MINH = 128, FC_MAXH = FC_OV + 1;
constexpr int FC_LDS = FC_N + FC_N / 16;  // one pad element per 16: every pass reads and writes conflict-free

__device__ __forceinline__ int fc_pad(int i) { return i + (i >> 4); }
__device__ __forceinline__ cf fc_conj(cf a) { return a * cf{1.0f, -1.0f}; }

template <bool INV>
__device__ __forceinline__ void fc_fft16(cf (&v)[16]) {  // INV: sum_k v[k] w16^(-q k) = conj(FFT(conj v))
  if (INV) {
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = fc_conj(v[j]);
  }
  fft16<false>(v);
  if (INV) {
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = fc_conj(v[j]);
  }
}

// tw[j] = e^(-2 pi i j / 4096)
__global__ __launch_bounds__(256) void fc_twiddle_kernel(cf* __restrict__ tw) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  double s, c;
  sincospi((double)j / 2048.0, &s, &c);
  tw[j] = cf{(float)c, (float)-s};
}

// Forward transform.  In: v[j] = z[256 j + t].  Out: v[k3] = Z[k1 + 16 k2 + 256 k3] with k1 = t >> 4, k2 = t & 15 - the
// spectrum element that lives at position 256 k1 + 16 k2 + k3 ("digit-reversed").
__device__ __forceinline__ void fc_forward(cf (&v)[16], cf* __restrict__ buf, const cf* __restrict__ tw, int t) {
  const int hi = t >> 4, lo = t & 15;
  fft16<false>(v);  // over a (n = 256 a + b, b = t) -> k1
#pragma unroll
  for (int k = 1; k < 16; ++k) v[k] = cmul(v[k], tw[t * k]);  // w4096^(b k1)
#pragma unroll
  for (int k = 0; k < 16; ++k) buf[fc_pad(k * 256 + t)] = v[k];
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 16; ++c) v[c] = buf[fc_pad(hi * 256 + 16 * c + lo)];  // k1 = hi, b = 16 c + d, d = lo
  fft16<false>(v);  // over c -> k2
#pragma unroll
  for (int k = 1; k < 16; ++k) v[k] = cmul(v[k], tw[16 * lo * k]);  // w256^(d k2)
#pragma unroll
  for (int k = 0; k < 16; ++k) buf[fc_pad(hi * 256 + 16 * k + lo)] = v[k];  // (the positions this thread has just read)
  __syncthreads();
#pragma unroll
  for (int d = 0; d < 16; ++d) v[d] = buf[fc_pad(hi * 256 + 16 * lo + d)];  // k1 = hi, k2 = lo
  fft16<false>(v);  // over d -> k3
}

// Inverse of fc_forward (unscaled).  In: v[k3] as fc_forward leaves it.  Out: v[a] = sum over the spectrum for n = 256 a + t.
__device__ __forceinline__ void fc_inverse(cf (&v)[16], cf* __restrict__ buf, const cf* __restrict__ tw, int t) {
  const int hi = t >> 4, lo = t & 15;
  fc_fft16<true>(v);  // over k3 -> d
#pragma unroll
  for (int d = 1; d < 16; ++d) v[d] = cmul(v[d], fc_conj(tw[16 * d * lo]));  // w256^(-d k2), k2 = lo
#pragma unroll
  for (int d = 0; d < 16; ++d) buf[fc_pad(hi * 256 + 16 * lo + d)] = v[d];  // (read by this thread only, in fc_forward)
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 16; ++k) v[k] = buf[fc_pad(hi * 256 + 16 * k + lo)];  // k1 = hi, d = lo, over k2
  fc_fft16<true>(v);  // -> c
#pragma unroll
  for (int c = 0; c < 16; ++c)
    if (16 * c + lo > 0) v[c] = cmul(v[c], fc_conj(tw[(16 * c + lo) * hi]));  // w4096^(-b k1)
#pragma unroll
  for (int c = 0; c < 16; ++c) buf[fc_pad(hi * 256 + 16 * c + lo)] = v[c];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 16; ++k) v[k] = buf[fc_pad(k * 256 + t)];  // b = t, over k1
  fc_fft16<true>(v);  // -> a
}

// spectra of the impulse responses, in fc_forward's order, scaled by 1 / 4096 (the inverse is unscaled)
__global__ __launch_bounds__(FC_NT) void fc_spectrum_kernel(const float* __restrict__ irs, int H, const cf* __restrict__ tw,
                                                            cf* __restrict__ spec) {
  __shared__ cf buf[FC_LDS];
  const int t = threadIdx.x;
  const float* __restrict__ h = irs + (size_t)blockIdx.x * H;
  cf v[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int n = 256 * j + t;
    v[j] = cf{n < H ? h[n] : 0.0f, 0.0f};
  }
  fc_forward(v, buf, tw, t);
  cf* __restrict__ o = spec + (size_t)blockIdx.x * FC_N + 16 * t;
#pragma unroll
  for (int k = 0; k < 16; ++k) o[k] = v[k] * (1.0f / (float)FC_N);
}

// The pair of output blocks (2 p, 2 p + 1), p = pair, of one utterance (baseA = 2 p FC_V < L) against ONE spectrum hs (the
// response's, at this thread's 16 elements): shared by fc_convolve_kernel and, for the rows of a bank that drew a response
// of at most FC_MAXH taps, by pb_convolve_kernel - the same statements, so those rows carry the same bits.
template <typename T>
__device__ __forceinline__ void fc_convolve_pair(const T* __restrict__ xb, float* __restrict__ yb, int L, int Lcap, int pair,
                                                 const cf* __restrict__ hs, const cf* __restrict__ tw, cf* __restrict__ buf,
                                                 unsigned* __restrict__ peaks, int b, int t) {
  const int baseA = 2 * pair * FC_V, baseB = baseA + FC_V;  // first output sample of either block
  cf v[16];
  float xpeak = 0.0f;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int mA = baseA - FC_OV + 256 * j + t, mB = mA + FC_V;
    const float a = (mA >= 0 && mA < L) ? air_pcm_sample(xb, mA) : 0.0f;
    const float c = mB < L ? air_pcm_sample(xb, mB) : 0.0f;
    v[j] = cf{a, c};
    if (j >= FC_OV / 256) xpeak = fmaxf(xpeak, fmaxf(fabsf(a), fabsf(c)));  // the blocks' own samples
  }
  fc_forward(v, buf, tw, t);
#pragma unroll
  for (int k = 0; k < 16; ++k) v[k] = cmul(v[k], hs[k]);
  fc_inverse(v, buf, tw, t);
  float ypeak = 0.0f;
#pragma unroll
  for (int a = FC_OV / 256; a < 16; ++a) {  // the samples behind the history: block A in the real, block B in the imaginary part
    const int o = 256 * a + t - FC_OV;
    if (baseA + o < L) {
      yb[baseA + o] = v[a][0];
      ypeak = fmaxf(ypeak, fabsf(v[a][0]));
    } else if (baseA + o < Lcap) {
      yb[baseA + o] = 0.0f;
    }
    if (baseB + o < L) {
      yb[baseB + o] = v[a][1];
      ypeak = fmaxf(ypeak, fabsf(v[a][1]));
    } else if (baseB + o < Lcap) {
      yb[baseB + o] = 0.0f;
    }
  }
  if (peaks) {
    xpeak = air_wave_max(xpeak);
    ypeak = air_wave_max(ypeak);
    if ((t & 63) == 0) {
      atomic_max_pos(peaks + 2 * b, xpeak);
      atomic_max_pos(peaks + 2 * b + 1, ypeak);
    }
  }
}

// blockIdx.x = pair of output blocks (2 p, 2 p + 1) of utterance blockIdx.y
template <typename T>
__global__ __launch_bounds__(FC_NT) void fc_convolve_kernel(const T* __restrict__ x, int Lcap, const int* __restrict__ lengths,
                                                            const cf* __restrict__ spec, const cf* __restrict__ tw,
                                                            const int* __restrict__ idx, float* __restrict__ y,
                                                            unsigned* __restrict__ peaks, int n_ir) {
  __shared__ cf buf[FC_LDS];
  const int b = blockIdx.y, t = threadIdx.x;
  const int L = air_row_len(lengths, b, Lcap);
  const T* __restrict__ xb = x + (size_t)b * Lcap;
  float* __restrict__ yb = y + (size_t)b * Lcap;
  const int ir = idx ? min(idx[b], n_ir - 1) : 0;
  if (ir < 0 || 2 * (int)blockIdx.x * FC_V >= L) {  // pass-through utterance, or a pair wholly behind the row's length: zeros
    ir_copy_span(xb, yb, 2 * (int)blockIdx.x * FC_V, 2 * FC_V, L, Lcap, t, FC_NT);
    return;
  }
  fc_convolve_pair(xb, yb, L, Lcap, (int)blockIdx.x, spec + (size_t)ir * FC_N + 16 * t, tw, buf, peaks, b, t);
}

inline size_t fc_align(size_t v) { return (v + 255) & ~(size_t)255; }
inline bool fc_wanted(int H) { return air_opt(AIR_OPT_IR_FFT) != 0 && H >= FC_MINH && H <= FC_MAXH; }

// Both entry points, arguments already checked.  lengths NULL: every row holds L samples (the dense call).
template <typename T>
int ir_launch(const T* x, int B, int L, const int* lengths, const float* irs, int n_ir, int H, const int* ir_idx,
              int normalize, float* y, void* ws, size_t ws_bytes, hipStream_t st) {
  unsigned* peaks = normalize ? reinterpret_cast<unsigned*>(ws) : nullptr;
  if (peaks && hipMemsetAsync(peaks, 0, (size_t)B * 2 * sizeof(unsigned), st) != hipSuccess) return AIR_ELAUNCH;
  if (fc_wanted(H) && ws && ws_bytes >= air_ir_convolve_ws_bytes_ex(B, n_ir, H)) {
    // (the tables are rebuilt per call - 16 + n_ir small workgroups - rather than cached against a bank the caller may
    // rewrite in place)
    char* base = reinterpret_cast<char*>(ws) + fc_align(air_ir_convolve_ws_bytes(B));
    cf* tw = reinterpret_cast<cf*>(base);
    cf* spec = reinterpret_cast<cf*>(base + fc_align((size_t)FC_N * sizeof(cf)));
    hipLaunchKernelGGL(fc_twiddle_kernel, dim3(FC_N / 256), dim3(256), 0, st, tw);
    AIR_CHECK_LAUNCH();
    hipLaunchKernelGGL(fc_spectrum_kernel, dim3(n_ir), dim3(FC_NT), 0, st, irs, H, tw, spec);
    AIR_CHECK_LAUNCH();
    const int nblk = (L + FC_V - 1) / FC_V;
    hipLaunchKernelGGL(fc_convolve_kernel<T>, dim3((nblk + 1) / 2, B), dim3(FC_NT), 0, st, x, L, lengths, spec, tw, ir_idx, y,
                       peaks, n_ir);
    AIR_CHECK_LAUNCH();
  } else {
    const dim3 grid((L + FIR_BLK - 1) / FIR_BLK, B);
    hipLaunchKernelGGL(fir_kernel<T>, grid, dim3(FIR_NT), 0, st, x, L, lengths, irs, H, ir_idx, y, peaks, n_ir);
    AIR_CHECK_LAUNCH();
  }
  if (normalize) {
    hipLaunchKernelGGL(fir_rescale_kernel, dim3(16, B), dim3(256), 0, st, y, L, lengths, ir_idx, peaks);
    AIR_CHECK_LAUNCH();
  }
  return AIR_OK;
}

// ---- G.711 transmission codec (air_g711_ragged) ----------------------------------------------------------------------
// 16 kHz -> low-pass, every second sample (8 kHz) -> 16-bit -> G.711 code -> 16-bit -> zero-stuff, low-pass -> 16 kHz, per
// row over its own L_b samples (include/air_hip.h has the arithmetic).  A byte mover (4 or 2 bytes in, 4 out per sample),
// so one workgroup takes a tile of GC_T outputs from global memory to global memory and keeps everything between in LDS:
//   * it stages x[n0 - 2c - pc, n0 + GC_T + 2c) - its tile plus the halo of BOTH filters - split by parity into E / O:
//     with the base chosen so that base + c is even, the even taps of the decimator read E and the odd taps O, both at
//     unit stride;
//   * it computes the GC_T / 2 + c 8 kHz samples its outputs need (the c of the halo are recomputed, not exchanged): a
//     thread owns GC_VR = 5 consecutive ones (stride 5 over the lanes: no LDS bank is hit twice) behind two sliding
//     register windows, one LDS read and GC_VR FMAs per tap, taps in ascending order into ONE accumulator; quantises,
//     codes and decodes them (decode: a 256-entry table of d / 32768 in LDS) and leaves v in LDS;
//   * it interpolates in polyphase form: a thread owns 8 consecutive outputs, the four whose (n + c) is even take the even
//     taps and the other four the odd taps, off one sliding window of v - the stuffed zeros are never multiplied;
//   * the outputs cross LDS once more so that the store is coalesced whatever Lcap's alignment.
// Nothing in the arithmetic depends on Lcap or on the other rows, so row b of a ragged batch carries the bits of the call
// on that utterance alone.
constexpr int GC_NT = 256, GC_R = 8, GC_T = GC_NT * GC_R;  // outputs per workgroup
constexpr int GC_MAXTAPS = 127, GC_MAXC = (GC_MAXTAPS - 1) / 2;
constexpr int GC_VR = 5;       // 8 kHz samples per thread: GC_NT * GC_VR >= GC_T / 2 + GC_MAXC
constexpr int GC_XH = 1168;    // floats per parity plane: >= GC_T / 2 + 2 GC_MAXC + GC_VR + 1; = 16 mod 32, so a wave's
                               // staging stores (even lanes -> E, odd lanes -> O) fall on 32 different banks
constexpr int GC_VS = 1104;    // v: one zero in front + GC_T / 2 + GC_MAXC samples, rounded up to whole threads
static_assert(GC_XH >= GC_T / 2 + 2 * GC_MAXC + GC_VR + 1 && GC_XH % 32 == 16, "parity planes");
static_assert(GC_VS >= 1 + GC_T / 2 + GC_MAXC + GC_VR && GC_NT * GC_VR >= GC_T / 2 + GC_MAXC, "8 kHz samples");
static_assert(GC_T <= 2 * GC_XH && GC_NT == 256, "the outputs reuse the planes; one thread per table entry");

__device__ __forceinline__ int g711_quantise(float u) {  // clamp(rint(u * 32768)): ties to even; NaN -> -32768
  return (int)fminf(fmaxf(rintf(u * 32768.0f), -32768.0f), 32767.0f);
}

// the tile [n0, n0 + GC_T) of a row that is copied (pass-through) or lies behind its length: y, and zero codes
template <typename T>
__device__ __forceinline__ void g711_skip_tile(const T* __restrict__ xb, float* __restrict__ yb, unsigned char* __restrict__ cb,
                                               int n0, int L, int Lcap, int c0, int cspan, int Ccap, int t) {
  ir_copy_span(xb, yb, n0, GC_T, L, Lcap, t, GC_NT);
  if (cb)
    for (int m = c0 + t; m < min(c0 + cspan, Ccap); m += GC_NT) cb[m] = 0;
}

// PC = c & 1.  ae[r] -> y[nb + 2 r + PC] (even taps), ao[r] -> y[nb + 2 r + 1 - PC] (odd taps); w[i] = v at LDS index wb + i - j
template <bool PC>
__device__ __forceinline__ void g711_interp(const float* __restrict__ vs, const float* __restrict__ hs, int c, int wb,
                                            float* __restrict__ o) {
  float w[5], ae[4] = {0.0f, 0.0f, 0.0f, 0.0f}, ao[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int i = 0; i < 5; ++i) w[i] = vs[wb + i];
  for (int j = 0; j < c; ++j) {
    const float he = hs[2 * j], ho = hs[2 * j + 1];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      ae[r] = fmaf(he, w[r + 1], ae[r]);
      ao[r] = fmaf(ho, PC ? w[r] : w[r + 1], ao[r]);
    }
#pragma unroll
    for (int i = 4; i > 0; --i) w[i] = w[i - 1];
    w[0] = vs[wb - j - 1];
  }
  const float he = hs[2 * c];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    ae[r] = fmaf(he, w[r + 1], ae[r]);
    o[2 * r + (PC ? 1 : 0)] = 2.0f * ae[r];
    o[2 * r + (PC ? 0 : 1)] = 2.0f * ao[r];
  }
}

template <typename T>
__global__ __launch_bounds__(GC_NT) void g711_resample_kernel(const T* __restrict__ x, int Lcap, const int* __restrict__ lengths,
                                                              const float* __restrict__ fir, int ntaps,
                                                              const int* __restrict__ law_idx, float* __restrict__ y,
                                                              unsigned char* __restrict__ codes, unsigned* __restrict__ peaks) {
  __shared__ __attribute__((aligned(16))) float xs[2 * GC_XH];  // E = xs, O = xs + GC_XH (O[-1] is read into a window slot that is never used)
  __shared__ float vs[GC_VS];
  __shared__ float hs[GC_MAXTAPS + 1];
  __shared__ float dec[256];
  const int b = blockIdx.y, n0 = blockIdx.x * GC_T, t = threadIdx.x;
  const int L = air_row_len(lengths, b, Lcap), M = (L + 1) >> 1, Mcap = (Lcap + 1) >> 1;
  const T* __restrict__ xb = x + (size_t)b * Lcap;
  float* __restrict__ yb = y + (size_t)b * Lcap;
  unsigned char* __restrict__ cb = codes ? codes + (size_t)b * Mcap : nullptr;
  const int law = law_idx ? min(law_idx[b], 1) : 0;  // caller data: anything above 1 is A-law
  if (law < 0 || n0 >= L) {
    g711_skip_tile(xb, yb, cb, n0, L, Lcap, n0 >> 1, GC_T / 2, Mcap, t);
    return;
  }
  const int c = (ntaps - 1) >> 1, pc = c & 1;
  const int ib = n0 - 2 * c - pc;                 // first staged sample; ib + c is even
  const int mbase = (n0 - c + pc) / 2;            // first 8 kHz sample of the tile (exact: the numerator is even)
  const int D = (3 * c + pc - n0) / 2;            // tap 2 j of sample m reads E[m - j + D], tap 2 j + 1 O[m - j + D - 1]
  const int NV = GC_T / 2 + c;
  float xpeak = 0.0f;
  for (int p = t; p < min(2 * GC_XH, GC_T + 4 * c + 12); p += GC_NT) {
    const int i = ib + p;
    const float v = (i >= 0 && i < L) ? air_pcm_sample(xb, i) : 0.0f;
    xs[(p & 1) * GC_XH + (p >> 1)] = v;
    if (i >= n0 && i < n0 + GC_T) xpeak = fmaxf(xpeak, fabsf(v));  // this tile's own samples
  }
  if (t < ntaps) hs[t] = fir[t];
  dec[t] = (float)g711_decode(law, t) * (1.0f / 32768.0f);
  if (t == 0) vs[0] = 0.0f;
  __syncthreads();

  for (int jv = t * GC_VR; jv < NV; jv += GC_NT * GC_VR) {
    const float* __restrict__ E = xs + (mbase + jv + D);
    const float* __restrict__ O = E + GC_XH - 1;
    float we[GC_VR], wo[GC_VR], u[GC_VR];
#pragma unroll
    for (int r = 0; r < GC_VR; ++r) {
      we[r] = E[r];
      wo[r] = O[r];
      u[r] = 0.0f;
    }
    for (int j = 0; j < c; ++j) {
      const float he = hs[2 * j], ho = hs[2 * j + 1];
#pragma unroll
      for (int r = 0; r < GC_VR; ++r) {
        u[r] = fmaf(he, we[r], u[r]);
        u[r] = fmaf(ho, wo[r], u[r]);
      }
#pragma unroll
      for (int r = GC_VR - 1; r > 0; --r) {
        we[r] = we[r - 1];
        wo[r] = wo[r - 1];
      }
      we[0] = E[-j - 1];
      wo[0] = O[-j - 1];
    }
    const float he = hs[2 * c];
#pragma unroll
    for (int r = 0; r < GC_VR; ++r) {
      const int m = mbase + jv + r;
      const bool live = m >= 0 && m < M;
      const int code = g711_encode(law, g711_quantise(fmaf(he, we[r], u[r])));
      vs[1 + jv + r] = live ? dec[code] : 0.0f;
      if (cb && m >= (n0 >> 1) && m < (n0 >> 1) + GC_T / 2 && m < Mcap) cb[m] = live ? (unsigned char)code : 0;
    }
  }
  __syncthreads();

  float o[GC_R];
  if (pc)
    g711_interp<true>(vs, hs, c, 4 * t + c, o);
  else
    g711_interp<false>(vs, hs, c, 4 * t + c, o);
  // (the planes were last read ahead of the barrier above)
  reinterpret_cast<float4*>(xs)[2 * t] = make_float4(o[0], o[1], o[2], o[3]);
  reinterpret_cast<float4*>(xs)[2 * t + 1] = make_float4(o[4], o[5], o[6], o[7]);
  __syncthreads();
  float ypeak = 0.0f;
  for (int i = t; i < GC_T && n0 + i < Lcap; i += GC_NT) {
    const float v = n0 + i < L ? xs[i] : 0.0f;
    yb[n0 + i] = v;
    ypeak = fmaxf(ypeak, fabsf(v));
  }
  if (peaks) {
    xpeak = air_wave_max(xpeak);
    ypeak = air_wave_max(ypeak);
    if ((t & 63) == 0) {
      atomic_max_pos(peaks + 2 * b, xpeak);
      atomic_max_pos(peaks + 2 * b + 1, ypeak);
    }
  }
}

// resample = 0: every sample is quantised, coded and decoded at its own rate
template <typename T>
__global__ __launch_bounds__(GC_NT) void g711_code_kernel(const T* __restrict__ x, int Lcap, const int* __restrict__ lengths,
                                                          const int* __restrict__ law_idx, float* __restrict__ y,
                                                          unsigned char* __restrict__ codes, unsigned* __restrict__ peaks) {
  const int b = blockIdx.y, n0 = blockIdx.x * GC_T, t = threadIdx.x;
  const int L = air_row_len(lengths, b, Lcap);
  const T* __restrict__ xb = x + (size_t)b * Lcap;
  float* __restrict__ yb = y + (size_t)b * Lcap;
  unsigned char* __restrict__ cb = codes ? codes + (size_t)b * Lcap : nullptr;
  const int law = law_idx ? min(law_idx[b], 1) : 0;
  if (law < 0 || n0 >= L) {
    g711_skip_tile(xb, yb, cb, n0, L, Lcap, n0, GC_T, Lcap, t);
    return;
  }
  float xpeak = 0.0f, ypeak = 0.0f;
  for (int n = n0 + t; n < min(n0 + GC_T, Lcap); n += GC_NT) {
    float v = 0.0f;
    int code = 0;
    if (n < L) {
      const float s = air_pcm_sample(xb, n);
      code = g711_encode(law, g711_quantise(s));
      v = (float)g711_decode(law, code) * (1.0f / 32768.0f);
      xpeak = fmaxf(xpeak, fabsf(s));
      ypeak = fmaxf(ypeak, fabsf(v));
    }
    yb[n] = v;
    if (cb) cb[n] = (unsigned char)code;
  }
  if (peaks) {
    xpeak = air_wave_max(xpeak);
    ypeak = air_wave_max(ypeak);
    if ((t & 63) == 0) {
      atomic_max_pos(peaks + 2 * b, xpeak);
      atomic_max_pos(peaks + 2 * b + 1, ypeak);
    }
  }
}

__global__ __launch_bounds__(256) void g711_clear_peaks_kernel(unsigned* __restrict__ peaks, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) peaks[i] = 0u;
}

template <typename T>
int g711_launch(const T* x, int B, int Lcap, const int* lengths, const float* fir, int ntaps, const int* law_idx, int resample,
                int normalize, float* y, uint8_t* codes, void* ws, hipStream_t st) {
  unsigned* peaks = normalize ? reinterpret_cast<unsigned*>(ws) : nullptr;
  if (peaks) {
    // a kernel, not hipMemsetAsync: this call is meant to be captured, and the memset node of these few bytes was seen to
    // write a non-zero pattern from the second replay of the graph on (tests/test_codec_gpu.py replays three times)
    hipLaunchKernelGGL(g711_clear_peaks_kernel, dim3((2 * B + 255) / 256), dim3(256), 0, st, peaks, 2 * B);
    AIR_CHECK_LAUNCH();
  }
  const dim3 grid((Lcap + GC_T - 1) / GC_T, B);
  if (resample)
    hipLaunchKernelGGL(g711_resample_kernel<T>, grid, dim3(GC_NT), 0, st, x, Lcap, lengths, fir, ntaps, law_idx, y, codes, peaks);
  else
    hipLaunchKernelGGL(g711_code_kernel<T>, grid, dim3(GC_NT), 0, st, x, Lcap, lengths, law_idx, y, codes, peaks);
  AIR_CHECK_LAUNCH();
  if (normalize) {
    hipLaunchKernelGGL(fir_rescale_kernel, dim3(16, B), dim3(256), 0, st, y, Lcap, lengths, law_idx, peaks);
    AIR_CHECK_LAUNCH();
  }
  return AIR_OK;
}

// ---- bank of responses of different lengths (air_ir_bank_convolve) ---------------------------------------------------
// Row b draws response i = idx[b] of taps_i = clamp(ir_taps[i], 1, Hmax) taps (device data).  Two forms in one launch:
//   * taps_i <= FC_MAXH: fc_convolve_pair against the spectrum of the response's first partition - the statements, the
//     block geometry (two 3072-sample blocks per transform) and hence the bits of air_ir_convolve_ragged;
//   * longer: UNIFORMLY PARTITIONED overlap-save.  Geometry: transform N = 4096, partition length = hop = PB_P = 2048
//     (taps - 1 + hop = 4095 <= N), so the response is cut into ceil(taps_i / 2048) partitions h_p and output block k
//     (samples [2048 k, 2048 k + 2048)) is the last 2048 samples of IFFT(sum_p X_{k-p} H_p), X_s the transform of
//     "segment" s = samples [2048 (s - 1), 2048 (s + 1)).  Two real segments ride one complex transform as before; a
//     product with a (real response's) spectrum keeps them apart, so a packed spectrum serves every partition that needs
//     BOTH its segments: output blocks (2 j, 2 j + 1) take, for even p, the "even" packing Ze_m = (segment 2 m, 2 m + 1)
//     at m = j - p / 2 and, for odd p, the "odd" packing Zo_m = (segment 2 m - 1, 2 m) at m = j - (p - 1) / 2.
//     pb_forward_kernel transforms every packing of a long row ONCE into the workspace (the odd ones only for rows with
//     a second partition); pb_convolve_kernel accumulates Z H over the row's own partitions in ascending p in registers
//     (16 complex values per thread, as the transforms) and takes ONE inverse per pair of output blocks.  Which segments
//     share a transform depends on the sample index alone, and the sum runs over the row's own partitions, so the bits of
//     y[b, :L_b] do not depend on Lcap, B or the other rows.
// Spectra of both forms keep fc_forward's digit-reversed order; the tables (twiddles, partition spectra) are rebuilt per
// call, as in ir_launch.  Grids are sized by the host-known Lcap and Hmax; workgroups of partitions a response does not
// have, of packings a row does not need and of blocks behind L_b return at once (the last kind after writing zeros).
constexpr int PB_P = 2048;                 // partition length = hop of the long form
constexpr int PB_MAXH = 65536;             // 32 partitions
static_assert(2 * PB_P == FC_N && PB_P % 256 == 0, "partition + hop fill the transform");

__device__ __forceinline__ int pb_taps(const int* __restrict__ ir_taps, int ir, int Hmax) { return min(max(ir_taps[ir], 1), Hmax); }

// blockIdx.x = partition, blockIdx.y = response.  spec[(i * nparts + p) * FC_N ...] = FFT(h_i[2048 p, 2048 p + 2048) & 0) / 4096
__global__ __launch_bounds__(FC_NT) void pb_spectrum_kernel(const float* __restrict__ irs, int Hmax, const int* __restrict__ ir_taps,
                                                            const cf* __restrict__ tw, cf* __restrict__ spec, int nparts) {
  __shared__ cf buf[FC_LDS];
  const int t = threadIdx.x, i = blockIdx.y, p = blockIdx.x;
  const int taps = pb_taps(ir_taps, i, Hmax);
  if (p * PB_P >= taps) return;  // a partition this response does not have: never read
  const float* __restrict__ h = irs + (size_t)i * Hmax;
  cf v[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int n = p * PB_P + 256 * j + t;
    v[j] = cf{(j < PB_P / 256 && n < taps) ? h[n] : 0.0f, 0.0f};
  }
  fc_forward(v, buf, tw, t);
  cf* __restrict__ o = spec + ((size_t)i * nparts + p) * FC_N + 16 * t;
#pragma unroll
  for (int k = 0; k < 16; ++k) o[k] = v[k] * (1.0f / (float)FC_N);
}

// blockIdx.x = m, blockIdx.y = packing (0: Ze_m, 1: Zo_m), blockIdx.z = row.  zs[((b * nz + packing) * npair + m) * FC_N ...]
template <typename T>
__global__ __launch_bounds__(FC_NT) void pb_forward_kernel(const T* __restrict__ x, int Lcap, const int* __restrict__ lengths,
                                                           int Hmax, const int* __restrict__ ir_taps, const cf* __restrict__ tw,
                                                           const int* __restrict__ idx, cf* __restrict__ zs,
                                                           unsigned* __restrict__ peaks, int n_ir, int npair) {
  __shared__ cf buf[FC_LDS];
  const int t = threadIdx.x, m = blockIdx.x, odd = blockIdx.y, b = blockIdx.z;
  const int ir = idx ? min(idx[b], n_ir - 1) : 0;
  if (ir < 0) return;
  const int taps = pb_taps(ir_taps, ir, Hmax);
  if (taps <= FC_MAXH || (odd && taps <= PB_P)) return;  // the short form; a row without an odd partition
  const int L = air_row_len(lengths, b, Lcap);
  if (2 * m * PB_P >= L) return;  // no pair of output blocks of this row reaches back to m
  const T* __restrict__ xb = x + (size_t)b * Lcap;
  const int s0 = (2 * m - odd - 1) * PB_P;  // first sample of the real part's segment; the imaginary part's is PB_P further
  cf v[16];
  float xpeak = 0.0f;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int mA = s0 + 256 * j + t, mB = mA + PB_P;
    const float a = (mA >= 0 && mA < L) ? air_pcm_sample(xb, mA) : 0.0f;
    const float c = (mB >= 0 && mB < L) ? air_pcm_sample(xb, mB) : 0.0f;
    v[j] = cf{a, c};
    if (j >= PB_P / 256) xpeak = fmaxf(xpeak, fmaxf(fabsf(a), fabsf(c)));  // (even packing) blocks 2 m and 2 m + 1: every sample once
  }
  fc_forward(v, buf, tw, t);
  cf* __restrict__ o = zs + (((size_t)b * gridDim.y + odd) * npair + m) * FC_N + 16 * t;
#pragma unroll
  for (int k = 0; k < 16; ++k) o[k] = v[k];
  if (peaks && !odd) {
    xpeak = air_wave_max(xpeak);
    if ((t & 63) == 0) atomic_max_pos(peaks + 2 * b, xpeak);
  }
}

// blockIdx.x = pair of output blocks of utterance blockIdx.y: 3072-sample blocks for a short response, 2048 for a long one
template <typename T>
__global__ __launch_bounds__(FC_NT) void pb_convolve_kernel(const T* __restrict__ x, int Lcap, const int* __restrict__ lengths,
                                                            int Hmax, const int* __restrict__ ir_taps, const cf* __restrict__ spec,
                                                            const cf* __restrict__ zs, const cf* __restrict__ tw,
                                                            const int* __restrict__ idx, float* __restrict__ y,
                                                            unsigned* __restrict__ peaks, int n_ir, int nparts, int nz, int npair) {
  __shared__ cf buf[FC_LDS];
  const int b = blockIdx.y, t = threadIdx.x, j = blockIdx.x;
  const int L = air_row_len(lengths, b, Lcap);
  const T* __restrict__ xb = x + (size_t)b * Lcap;
  float* __restrict__ yb = y + (size_t)b * Lcap;
  const int ir = idx ? min(idx[b], n_ir - 1) : 0;
  const int taps = ir < 0 ? 1 : pb_taps(ir_taps, ir, Hmax);
  if (taps <= FC_MAXH) {  // pass-through and short rows: fc_convolve_kernel's tiling (spans past Lcap store nothing)
    if (ir < 0 || 2 * j * FC_V >= L)
      ir_copy_span(xb, yb, 2 * j * FC_V, 2 * FC_V, L, Lcap, t, FC_NT);
    else
      fc_convolve_pair(xb, yb, L, Lcap, j, spec + (size_t)ir * nparts * FC_N + 16 * t, tw, buf, peaks, b, t);
    return;
  }
  const int base = 2 * j * PB_P;
  if (base >= L) {  // a pair wholly behind the row's length: zeros
    ir_copy_span(xb, yb, base, 2 * PB_P, L, Lcap, t, FC_NT);
    return;
  }
  const int np = (taps + PB_P - 1) / PB_P;
  const cf* __restrict__ hrow = spec + (size_t)ir * nparts * FC_N + 16 * t;
  const cf* __restrict__ zrow = zs + (size_t)b * nz * npair * FC_N + 16 * t;
  cf v[16];
  {
    const cf* __restrict__ z = zrow + (size_t)j * FC_N;
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = cmul(z[k], hrow[k]);
  }
  for (int p = 1; p < np; ++p) {
    const int m = j - (p >> 1);
    if (m < 0) break;  // segments in front of the utterance: zero
    const cf* __restrict__ z = zrow + ((size_t)(p & 1) * npair + m) * FC_N;
    const cf* __restrict__ h = hrow + (size_t)p * FC_N;
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = v[k] + cmul(z[k], h[k]);
  }
  fc_inverse(v, buf, tw, t);
  float ypeak = 0.0f;
#pragma unroll
  for (int a = PB_P / 256; a < 16; ++a) {  // behind the history: block 2 j in the real, block 2 j + 1 in the imaginary part
    const int nA = base + 256 * a + t - PB_P, nB = nA + PB_P;
    if (nA < L) {
      yb[nA] = v[a][0];
      ypeak = fmaxf(ypeak, fabsf(v[a][0]));
    } else if (nA < Lcap) {
      yb[nA] = 0.0f;
    }
    if (nB < L) {
      yb[nB] = v[a][1];
      ypeak = fmaxf(ypeak, fabsf(v[a][1]));
    } else if (nB < Lcap) {
      yb[nB] = 0.0f;
    }
  }
  if (peaks) {
    ypeak = air_wave_max(ypeak);
    if ((t & 63) == 0) atomic_max_pos(peaks + 2 * b + 1, ypeak);
  }
}

struct PbPlan {  // host-known geometry of one call
  int nparts, nz, npair, gx;
  size_t off_tw, off_spec, off_z, total;
};

inline PbPlan pb_plan(int B, int Lcap, int n_ir, int Hmax) {
  PbPlan g;
  g.nparts = (Hmax + PB_P - 1) / PB_P;
  g.nz = Hmax <= FC_MAXH ? 0 : (g.nparts > 1 ? 2 : 1);  // packings kept per row: none, even, even + odd
  g.npair = ((Lcap + PB_P - 1) / PB_P + 1) / 2;
  const int short_pairs = ((Lcap + FC_V - 1) / FC_V + 1) / 2;
  g.gx = g.nz ? (g.npair > short_pairs ? g.npair : short_pairs) : short_pairs;
  g.off_tw = fc_align(air_ir_convolve_ws_bytes(B));
  g.off_spec = g.off_tw + fc_align((size_t)FC_N * sizeof(cf));
  g.off_z = g.off_spec + (size_t)n_ir * g.nparts * FC_N * sizeof(cf);
  g.total = g.off_z + (size_t)B * g.nz * g.npair * FC_N * sizeof(cf);
  return g;
}

template <typename T>
int pb_launch(const T* x, int B, int Lcap, const int* lengths, const float* irs, int n_ir, int Hmax, const int* ir_taps,
              const int* ir_idx, int normalize, float* y, void* ws, hipStream_t st) {
  const PbPlan g = pb_plan(B, Lcap, n_ir, Hmax);
  char* base = reinterpret_cast<char*>(ws);
  unsigned* peaks = normalize ? reinterpret_cast<unsigned*>(ws) : nullptr;
  cf* tw = reinterpret_cast<cf*>(base + g.off_tw);
  cf* spec = reinterpret_cast<cf*>(base + g.off_spec);
  cf* zs = reinterpret_cast<cf*>(base + g.off_z);
  if (peaks) {  // (a kernel, not a memset: see g711_launch)
    hipLaunchKernelGGL(g711_clear_peaks_kernel, dim3((2 * B + 255) / 256), dim3(256), 0, st, peaks, 2 * B);
    AIR_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(fc_twiddle_kernel, dim3(FC_N / 256), dim3(256), 0, st, tw);
  AIR_CHECK_LAUNCH();
  hipLaunchKernelGGL(pb_spectrum_kernel, dim3(g.nparts, n_ir), dim3(FC_NT), 0, st, irs, Hmax, ir_taps, tw, spec, g.nparts);
  AIR_CHECK_LAUNCH();
  if (g.nz) {
    hipLaunchKernelGGL(pb_forward_kernel<T>, dim3(g.npair, g.nz, B), dim3(FC_NT), 0, st, x, Lcap, lengths, Hmax, ir_taps, tw,
                       ir_idx, zs, peaks, n_ir, g.npair);
    AIR_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(pb_convolve_kernel<T>, dim3(g.gx, B), dim3(FC_NT), 0, st, x, Lcap, lengths, Hmax, ir_taps, spec, zs, tw,
                     ir_idx, y, peaks, n_ir, g.nparts, g.nz, g.npair);
  AIR_CHECK_LAUNCH();
  if (normalize) {
    hipLaunchKernelGGL(fir_rescale_kernel, dim3(16, B), dim3(256), 0, st, y, Lcap, lengths, ir_idx, peaks);
    AIR_CHECK_LAUNCH();
  }
  return AIR_OK;
}

}  // namespace

extern "C" {

size_t air_ir_convolve_ws_bytes(int B) { return B > 0 ? (size_t)B * 2 * sizeof(unsigned) + 256 : 0; }

size_t air_ir_convolve_ws_bytes_ex(int B, int n_ir, int H) {
  if (B <= 0 || n_ir <= 0 || H <= 0) return 0;
  size_t n = fc_align(air_ir_convolve_ws_bytes(B));
  if (fc_wanted(H)) n += fc_align((size_t)FC_N * sizeof(cf)) + (size_t)n_ir * FC_N * sizeof(cf);
  return n;
}

int air_ir_convolve(const float* x, int B, int L, const float* irs, int n_ir, int H, const int* ir_idx,
                    int normalize, float* y, void* ws, size_t ws_bytes, air_stream_t stream) {
  if (!x || !y || !irs || B <= 0 || L <= 0 || n_ir <= 0 || H <= 0 || x == y) return AIR_EINVAL;
  if (normalize && (!ws || ws_bytes < air_ir_convolve_ws_bytes(B))) return AIR_EWORKSPACE;
  return ir_launch(x, B, L, nullptr, irs, n_ir, H, ir_idx, normalize, y, ws, ws_bytes, air_stream(stream));
}

int air_ir_convolve_ragged(const float* x, const int16_t* x16, int B, int Lcap, const int* lengths_dev,
                           const float* irs, int n_ir, int H, const int* ir_idx, int normalize,
                           float* y, void* ws, size_t ws_bytes, air_stream_t stream) {
  if ((x != nullptr) == (x16 != nullptr) || !lengths_dev || !y || !irs || B <= 0 || Lcap <= 0 || n_ir <= 0 || H <= 0 ||
      (x && x == y))
    return AIR_EINVAL;
  if (normalize && (!ws || ws_bytes < air_ir_convolve_ws_bytes(B))) return AIR_EWORKSPACE;
  hipStream_t st = air_stream(stream);
  if (x16)
    return ir_launch(reinterpret_cast<const short*>(x16), B, Lcap, lengths_dev, irs, n_ir, H, ir_idx, normalize, y, ws, ws_bytes, st);
  return ir_launch(x, B, Lcap, lengths_dev, irs, n_ir, H, ir_idx, normalize, y, ws, ws_bytes, st);
}

size_t air_g711_ws_bytes(int B) { return air_ir_convolve_ws_bytes(B); }  // the same two peaks per row

int air_g711_ragged(const float* x, const int16_t* x16, int B, int Lcap, const int* lengths_dev_or_null, const float* fir,
                    int ntaps, const int* law_idx, int resample, int normalize, float* y, uint8_t* codes_or_null, void* ws,
                    size_t ws_bytes, air_stream_t stream) {
  if ((x != nullptr) == (x16 != nullptr) || !y || B <= 0 || Lcap <= 0 || ntaps < 1 || ntaps > GC_MAXTAPS || !(ntaps & 1) ||
      (resample && !fir) || (x && x == y))
    return AIR_EINVAL;
  if (normalize && (!ws || ws_bytes < air_g711_ws_bytes(B))) return AIR_EWORKSPACE;
  hipStream_t st = air_stream(stream);
  if (x16)
    return g711_launch(reinterpret_cast<const short*>(x16), B, Lcap, lengths_dev_or_null, fir, ntaps, law_idx, resample,
                       normalize, y, codes_or_null, ws, st);
  return g711_launch(x, B, Lcap, lengths_dev_or_null, fir, ntaps, law_idx, resample, normalize, y, codes_or_null, ws, st);
}

size_t air_ir_bank_ws_bytes(int B, int Lcap, int n_ir, int Hmax) {
  if (B <= 0 || Lcap <= 0 || n_ir <= 0 || Hmax <= 0 || Hmax > PB_MAXH) return 0;
  return pb_plan(B, Lcap, n_ir, Hmax).total;
}

int air_ir_bank_convolve(const float* x, const int16_t* x16, int B, int Lcap, const int* lengths_dev_or_null, const float* irs,
                         int n_ir, int Hmax, const int* ir_taps_dev, const int* ir_idx, int normalize, float* y, void* ws,
                         size_t ws_bytes, air_stream_t stream) {
  if ((x != nullptr) == (x16 != nullptr) || !y || !irs || !ir_taps_dev || B <= 0 || B > 65535 || Lcap <= 0 || n_ir <= 0 ||
      n_ir > 65535 || Hmax <= 0 || Hmax > PB_MAXH || (x && x == y))
    return AIR_EINVAL;
  if (!ws || ws_bytes < air_ir_bank_ws_bytes(B, Lcap, n_ir, Hmax)) return AIR_EWORKSPACE;
  hipStream_t st = air_stream(stream);
  if (x16)
    return pb_launch(reinterpret_cast<const short*>(x16), B, Lcap, lengths_dev_or_null, irs, n_ir, Hmax, ir_taps_dev, ir_idx,
                     normalize, y, ws, st);
  return pb_launch(x, B, Lcap, lengths_dev_or_null, irs, n_ir, Hmax, ir_taps_dev, ir_idx, normalize, y, ws, st);
}

}  // extern "C"
