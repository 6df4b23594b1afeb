// Spectrogram front-ends for gfx950: the reference's STFT (feature_extraction.py:141-165, dumped by preprocess.py:35-47)
// and Melspec (feature_extraction.py:168-176 = librosa.feature.melspectrogram(sr=16000, n_fft=512, hop_length=128);
// preprocess.py:176-215, :247-258), each in ONE launch from PCM to the layout the models read.
//
//   STFT  pre-emphasis (:157, optional) -> 320-tap periodic Hamming window centred in 512 points, hop 160, 256 zeros
//         each side (torch.stft, :159-161) -> |X_k|^2, k = 0 .. 256 (:163).  T = 1 + L / 160, D = 257.
//   MEL   512-tap periodic Hann window, hop 128, 256 reflected or zero samples each side -> |X_k|^2 -> 128-band Slaney
//         mel filterbank with Slaney area normalisation.  T = 1 + L / 128, D = 128.  No log in either.
//
// Mapping (wave64), as in csrc/lfcc.hip: 16 lanes per frame, 4 frames per wave, 8 waves per workgroup.  There are no
// deltas, hence no halo: a workgroup computes and writes the same 32 frames.  The 512-point real FFT is a 256-point
// complex FFT on the even/odd packing, done as 16 x 16 with the radix-16 butterfly of air_fft16.h, the transpose through
// a padded wave-private LDS tile and the real-FFT untangle against lane (16 - g) of the same 16-lane group (the window /
// transpose / untangle are restated here: lfcc.hip's bits are pinned and that file is left alone).  The STFT window sits
// at offset 0 of the frame instead of 96: a phase only, which |X|^2 discards.
//
// LDS: every wave handles ONE 4-frame group, so the staged PCM is dead once each lane holds its 16 windowed samples - a
// barrier later the same bytes are the output tile, [D][32 + 1] floats for the (B, D, feat_len) layout (every (bin,
// 32-frame) run leaves as one 128-byte segment) or [32][D] for (B, T, D).  STFT: max(21.1 KB PCM, 33.9 KB tile) + 34.8
// KB of exchange tiles = 68.7 KB; MEL: max(17.9, 16.9) + 34.8 + 6.1 KB of filter weights = 58.9 KB: two workgroups
// per CU of 160 KB either way ("Spectrogram front-ends").
#include <math.h>
#include <string.h>

#include "air_common.h"
#include "air_fft16.h"
#include "air_pcm.h"

namespace {

constexpr int FN = 512;
constexpr int NBIN = FN / 2 + 1;      // 257
constexpr int NW = 8;                 // waves per workgroup
constexpr int NTHREADS = NW * 64;
constexpr int FT = 4 * NW;            // 32 frames computed and written per workgroup
constexpr int XROW = 17;              // padded transpose row (complex elements)
constexpr int PROW = 264;             // MEL: power-spectrum row stride; zeros behind the Nyquist bin
constexpr int XCH_FLOATS = 4 * 16 * XROW;  // wave-private: the 4 x 16 x 17 transposition, then (MEL) 4 power rows
static_assert(4 * PROW <= XCH_FLOATS, "power rows must fit the exchange tile");
constexpr int OSTR = FT + 1;          // (B, D, feat_len) layout: s_out[c][fo], odd stride
constexpr int NMEL = 128;             // mel bands: 8 per lane of a 16-lane frame group
constexpr int MELW = 12;              // bins per mel filter held in the banded table (the widest filter spans 12)

struct SpecPlan {
  int kind, D, hop, wlen, nbin, maxw, pad0, pad1;
  float window[FN];           // STFT: 320 taps then zeros; MEL: 512 taps
  float tw256[512];           // e^{-2 pi i n/256}: (re, im), n = 0..255
  float tw512[32];            // e^{-2 pi i q/512}: (re, im), q = 0..15
  int lo[NMEL];               // MEL: first bin of filter j
  int cnt[NMEL];              // MEL: bins spanned by filter j
  float fbwT[MELW * NMEL];    // MEL: [i][j] = weight of bin lo[j] + i in filter j
};

__device__ __constant__ const float W32C[16] = {
    1.000000000f, 0.980785280f, 0.923879533f, 0.831469612f, 0.707106781f, 0.555570233f,
    0.382683432f, 0.195090322f, 0.000000000f, -0.195090322f, -0.382683432f, -0.555570233f,
    -0.707106781f, -0.831469612f, -0.923879533f, -0.980785280f};
__device__ __constant__ const float W32S[16] = {
    0.000000000f, 0.195090322f, 0.382683432f, 0.555570233f, 0.707106781f, 0.831469612f,
    0.923879533f, 0.980785280f, 1.000000000f, 0.980785280f, 0.923879533f, 0.831469612f,
    0.707106781f, 0.555570233f, 0.382683432f, 0.195090322f};

template <int KIND>
struct Geo;
template <>
struct Geo<AIR_SPEC_STFT> {
  static constexpr int HOP = 160, D = NBIN, LEAD = 160, NM = 10;  // NM: live radix-16 input rows (320 taps = 160 complex)
  static constexpr int NSAMP = HOP * (FT - 1) + 320;              // 5,280 staged samples
};
template <>
struct Geo<AIR_SPEC_MEL> {
  static constexpr int HOP = 128, D = NMEL, LEAD = 256, NM = 16;  // all sixteen rows live
  static constexpr int NSAMP = HOP * (FT - 1) + FN;               // 4,480 staged samples
};

struct SpecArgs {
  const float* pcm;
  const short* pcm16;   // non-null: 16-bit PCM, x = s / 32768 (exact)
  float* out;
  const SpecPlan* plan;
  const int* start;     // padded layout: per-row crop start (may be null)
  const int* lengths;   // padded layout: per-row samples (null: every row holds L), clamped to [1, L] on the device
  int L, T, tiles, flags, feat_len, pad_mode;
};

constexpr int FLAG_EMPH = AIR_SPEC_EMPHASIS;
constexpr int FLAG_REFLECT = AIR_SPEC_REFLECT;

constexpr int cmax(int a, int b) { return a > b ? a : b; }

// PADDED: out is (B, D, feat_len), rows may be ragged (a.lengths) and chopped (a.start); otherwise (B, T, D).
template <int KIND, bool PADDED>
__global__ __launch_bounds__(NTHREADS, 2) void spec_kernel(SpecArgs a) {
  using G = Geo<KIND>;
  constexpr int HOP = G::HOP, D = G::D, NSAMP = G::NSAMP, NM = G::NM;
  constexpr bool MEL = KIND == AIR_SPEC_MEL;
  constexpr int MAIN = cmax(NSAMP, PADDED ? D * OSTR : FT * D);
  // the staged PCM, then (behind the barrier that ends its life) the output tile
  __shared__ __attribute__((aligned(16))) float s_main[(MAIN + 3) & ~3];
  __shared__ __attribute__((aligned(16))) float s_xch[NW * XCH_FLOATS];
  __shared__ float s_fbw[MEL ? MELW * NMEL : 1];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int b = blockIdx.x / a.tiles;
  const int tile = blockIdx.x - b * a.tiles;
  const int t0 = tile * FT;
  const SpecPlan* __restrict__ plan = a.plan;
  if (plan->kind != KIND) return;  // a plan of the other kind: nothing is written (workgroup-uniform)
  int L = a.L, T = a.T;
  int live_tiles = a.tiles;  // tiles of this row that write frames: they share the row's zero frames
  if constexpr (PADDED) {
    if (a.lengths != nullptr) L = min(max(a.lengths[b], 1), a.L);  // a bad length in device memory stays inside the row
    T = 1 + L / HOP;
    live_tiles = (T + FT - 1) / FT;
    bool dead = t0 >= T;  // this tile holds no frame that the row writes
    if (T > a.feat_len) {
      // chopped row: only the tiles that overlap [start, start + feat_len) are written (same clamp as below)
      const int st = a.start != nullptr ? min(max(a.start[b], 0), T - a.feat_len) : 0;
      dead = dead || t0 + FT <= st || t0 >= st + a.feat_len;
    }
    if (dead) return;  // (workgroup-uniform, ahead of every barrier and of the staging)
  }
  const float* __restrict__ row = a.pcm ? a.pcm + (size_t)b * a.L : nullptr;
  const short* __restrict__ row16 = a.pcm16 ? a.pcm16 + (size_t)b * a.L : nullptr;
  auto sample = [&](long m) -> float { return row16 ? air_pcm_sample(row16, m) : row[m]; };

  // ---- stage the filter weights and the PCM --------------------------------
  if constexpr (MEL) {
    for (int e = tid; e < MELW * NMEL; e += NTHREADS) s_fbw[e] = plan->fbwT[e];
  }
  const long s0 = (long)HOP * t0 - G::LEAD;  // first staged sample (may be < 0); a multiple of 4
  const bool emph = !MEL && (a.flags & FLAG_EMPH) != 0;
  const bool reflect = MEL && (a.flags & FLAG_REFLECT) != 0;
  const bool vec_ok = row16 == nullptr && ((((size_t)row) & 15) == 0);
  for (int e4 = tid; e4 < NSAMP / 4; e4 += NTHREADS) {
    const long n = s0 + 4 * (long)e4;
    float v[4];
    if (vec_ok && n >= 0 && n + 3 < L) {
      const float4 q = *reinterpret_cast<const float4*>(row + n);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
      if (emph) {
        const float prev = n > 0 ? row[n - 1] : 0.0f;
        // non-recursive FIR on the ORIGINAL samples, two roundings like the reference (:157)
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
        if (reflect) {
          // numpy's "reflect": x[-m] in front, x[2 (L - 1) - m] behind; one reflection, then clamped into the row - what
          // a frame of a row of at least 257 samples reads is never clamped, and nothing can read outside a shorter one
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
    *reinterpret_cast<float4*>(&s_main[4 * e4]) = make_float4(v[0], v[1], v[2], v[3]);
  }

  // ---- per-lane constants --------------------------------------------------
  const int f = lane >> 4;       // frame within the wave's 4-frame group
  const int g = lane & 15;       // lane within the frame
  const int fi = wave * 4 + f;   // frame within the tile
  const bool active = t0 + wave * 4 < T;  // wave-uniform: the group holds a frame of the row
  const float cq = plan->tw512[2 * g];        //  cos(2 pi g/512)
  const float sq = -plan->tw512[2 * g + 1];   //  sin(2 pi g/512)
  const int partner = (lane & 48) | ((16 - g) & 15);
  float* xch = s_xch + wave * XCH_FLOATS;

  __syncthreads();

  // windowed even/odd packing: z[n] = w[2n] s[2n] + i w[2n+1] s[2n+1], n = g + 16 m
  cf x[16];
  if (active) {
#pragma unroll
    for (int m = 0; m < NM; ++m) {
      const float2 s = *reinterpret_cast<const float2*>(&s_main[HOP * fi + 2 * (g + 16 * m)]);
      const float2 w = *reinterpret_cast<const float2*>(&plan->window[2 * (g + 16 * m)]);
      x[m] = cf{s.x * w.x, s.y * w.y};
    }
#pragma unroll
    for (int m = NM; m < 16; ++m) x[m] = cf{0.0f, 0.0f};
  }
  __syncthreads();  // every frame is in registers: s_main is the output tile from here on
  float* __restrict__ s_out = s_main;

  if (active) {
    fft16<NM == 10>(x);  // over m: Y[g][q]  (STFT: rows 10..15 are zero and pruned)
#pragma unroll
    for (int q = 1; q < 16; ++q) {
      const int n = (g * q) & 255;
      x[q] = cmul(x[q], cf{plan->tw256[2 * n], plan->tw256[2 * n + 1]});  // w256^(g q)
    }
    // transpose through LDS: row q, column g - real parts, then imaginary parts through the same 4.3 KB
    float xre[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) xch[(f * 16 + q) * XROW + g] = x[q].x;
    air_wave_lds_fence();
#pragma unroll
    for (int l = 0; l < 16; ++l) xre[l] = xch[(f * 16 + g) * XROW + l];
    air_wave_lds_fence();
#pragma unroll
    for (int q = 0; q < 16; ++q) xch[(f * 16 + q) * XROW + g] = x[q].y;
    air_wave_lds_fence();
#pragma unroll
    for (int l = 0; l < 16; ++l) x[l] = cf{xre[l], xch[(f * 16 + g) * XROW + l]};
    fft16<false>(x);  // over l: Z[g + 16 p] = x[p]
    air_wave_lds_fence();  // MEL: the exchange tile is reused for the power rows below

    // where bin k of this lane's frame goes: the output tile (STFT) or the wave's power row (MEL)
    auto put = [&](int k, float pw) {
      if constexpr (MEL) xch[f * PROW + k] = pw;
      else if constexpr (PADDED) s_out[k * OSTR + fi] = pw;
      else s_out[fi * D + k] = pw;
    };
    // real-FFT untangle + power.  Partner lane holds Z[(16-g)%16 + 16 p'].
    float pnyq = 0.0f;
#pragma unroll
    for (int p = 0; p < 16; ++p) {
      // bin k = g + 16 p pairs with 256 - k: lane (16-g)&15, index 15-p  (g != 0)
      //                                      own lane, index (16-p)&15   (g == 0)
      const int pp = 15 - p;
      float bre = __shfl(x[pp].x, partner, 64);
      float bim = __shfl(x[pp].y, partner, 64);
      const int p0 = (16 - p) & 15;
      if (g == 0) {
        bre = x[p0].x;
        bim = x[p0].y;
      }
      // E2 = A + conj(B), O2 = A - conj(B);  2X = E2 - i w512^k O2
      const cf A = x[p], Bv = cf{bre, bim};
      const cf E = __builtin_elementwise_fma(Bv, cf{1.0f, -1.0f}, A);  // (A.re + bre, A.im - bim)
      const cf O = __builtin_elementwise_fma(Bv, cf{-1.0f, 1.0f}, A);  // (A.re - bre, A.im + bim)
      const cf cs = cmul(cf{cq, sq}, cf{W32C[p], W32S[p]});  // (cos, sin)(2 pi k / 512)
      const cf P1 = LFCC_LO(cs) * LFCC_SWAP(O);              // (c oim, c ore)
      const cf X1 = __builtin_elementwise_fma(P1, cf{1.0f, -1.0f}, E);
      const cf X = X1 - LFCC_HI(cs) * O;                     // - (s ore, s oim)
      const cf X2 = X * X;
      // the reference takes norm(., 2, -1).pow(2) (:163), fl(fl(sqrt(s))^2), within 1.5 ulp of s itself; the power is
      // taken directly (X holds 2 x the bin: the factor 0.25 is exact)
      put(g + 16 * p, 0.25f * (X2.x + X2.y));
      if (p == 0) {
        const float ny = x[0].x - x[0].y;  // X[256] = Re Z0 - Im Z0 (real)
        pnyq = ny * ny;
      }
    }
    if (g == 0) put(256, pnyq);

    if constexpr (MEL) {
      if (g >= 1 && g < PROW - 256) xch[f * PROW + 256 + g] = 0.0f;  // zeros behind the Nyquist bin
      air_wave_lds_fence();
      // banded mel filterbank: filter j = g + 16 i reads bins lo[j] .. lo[j] + MELW - 1 <= PROW - 1 (checked where the
      // plan is built); past its own support the weights are zero, past the Nyquist bin the row is zero
#pragma unroll
      for (int i = 0; i < NMEL / 16; ++i) {
        const int j = g + 16 * i;
        const float* __restrict__ pr = xch + f * PROW + plan->lo[j];
        float acc = 0.0f;
#pragma unroll
        for (int w = 0; w < MELW; ++w) acc = fmaf(pr[w], s_fbw[w * NMEL + j], acc);
        if constexpr (PADDED) s_out[j * OSTR + fi] = acc;
        else s_out[fi * D + j] = acc;
      }
    }
  }
  __syncthreads();

  // ---- coalesced stores ------------------------------------------------------
  if constexpr (!PADDED) {
    float* __restrict__ orow = a.out + ((size_t)b * T + t0) * D;
    const int n = min(FT, T - t0) * D;
    if ((D & 3) == 0 && ((reinterpret_cast<size_t>(orow) & 15) == 0)) {
      for (int e = tid; e < n / 4; e += NTHREADS)
        reinterpret_cast<float4*>(orow)[e] = reinterpret_cast<const float4*>(s_out)[e];
    } else {
      for (int e = tid; e < n; e += NTHREADS) orow[e] = s_out[e];
    }
  } else {
    // (B, D, feat_len): frame t lands on t' = t - start (+ k T when repeating); a 32-lane run is one bin's 32 frames
    const int flen = a.feat_len;
    // crop start clamped to the valid range: a bad offset must not leave columns unwritten
    const int start = (a.start != nullptr && T > flen) ? min(max(a.start[b], 0), T - flen) : 0;
    float* __restrict__ obase = a.out + (size_t)b * D * flen;
    const int npad = flen - T;  // > 0: pad (dataset.py:72-79)
    for (int e = tid; e < FT * D; e += NTHREADS) {
      const int c = e / FT, fo = e - c * FT;
      const int t = t0 + fo;
      if (t >= T) continue;
      const float v = s_out[c * OSTR + fo];
      if (T >= flen) {
        const int tp = t - start;
        if (tp >= 0 && tp < flen) obase[(size_t)c * flen + tp] = v;
      } else if (a.pad_mode == AIR_PAD_REPEAT) {
        for (int tp = t; tp < flen; tp += T) obase[(size_t)c * flen + tp] = v;
      } else {
        obase[(size_t)c * flen + t] = v;
      }
    }
    if (npad > 0 && a.pad_mode == AIR_PAD_ZERO) {
      // the npad zero frames appended (dataset.py:513-517), shared out over the row's live tiles
      for (int e = tile * NTHREADS + tid; e < npad * D; e += live_tiles * NTHREADS) {
        const int c = e / npad, k = e - c * npad;
        obase[(size_t)c * flen + T + k] = 0.0f;
      }
    }
  }
}

template <int KIND>
int spec_launch(const float* pcm, const short* pcm16, int B, int L, const int* lengths, float* out, int feat_len,
                const int* start, const void* plan_dev, int flags, int pad_mode, bool padded, hipStream_t stream) {
  constexpr int HOP = Geo<KIND>::HOP;
  SpecArgs a;
  a.pcm = pcm;
  a.pcm16 = pcm16;
  a.out = out;
  a.plan = reinterpret_cast<const SpecPlan*>(plan_dev);
  a.start = start;
  a.lengths = lengths;
  a.L = L;
  a.T = 1 + L / HOP;
  a.tiles = (a.T + FT - 1) / FT;
  a.flags = flags;
  a.feat_len = feat_len;
  a.pad_mode = pad_mode;
  if ((long)B * a.tiles > 0x7fffffffL) return AIR_EINVAL;
  const dim3 grid((unsigned)(B * a.tiles));
  if (padded)
    hipLaunchKernelGGL((spec_kernel<KIND, true>), grid, dim3(NTHREADS), 0, stream, a);
  else
    hipLaunchKernelGGL((spec_kernel<KIND, false>), grid, dim3(NTHREADS), 0, stream, a);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

int spec_flags(int kind, int flags) {
  return flags & (kind == AIR_SPEC_STFT ? AIR_SPEC_EMPHASIS : AIR_SPEC_REFLECT);
}

// Slaney mel scale (librosa.hz_to_mel / mel_to_hz, htk=False): linear at 200/3 Hz per mel below 1 kHz, log above
double mel_logstep() { return log(6.4) / 27.0; }
double hz_to_mel(double f) { return f >= 1000.0 ? 15.0 + log(f / 1000.0) / mel_logstep() : f / (200.0 / 3.0); }
double mel_to_hz(double m) { return m >= 15.0 ? 1000.0 * exp(mel_logstep() * (m - 15.0)) : (200.0 / 3.0) * m; }

}  // namespace

extern "C" {

size_t air_spec_plan_bytes(void) { return sizeof(SpecPlan); }

int air_spec_out_dim(int kind) { return kind == AIR_SPEC_STFT ? NBIN : (kind == AIR_SPEC_MEL ? NMEL : AIR_EINVAL); }

int air_spec_plan_build(int kind, void* plan_host_out) {
  if (!plan_host_out) return AIR_EINVAL;
  if (kind != AIR_SPEC_STFT && kind != AIR_SPEC_MEL) return AIR_EUNSUPPORTED;
  SpecPlan* p = reinterpret_cast<SpecPlan*>(plan_host_out);
  memset(p, 0, sizeof(SpecPlan));
  const bool mel = kind == AIR_SPEC_MEL;
  p->kind = kind;
  p->D = mel ? NMEL : NBIN;
  p->hop = mel ? Geo<AIR_SPEC_MEL>::HOP : Geo<AIR_SPEC_STFT>::HOP;
  p->wlen = mel ? FN : 320;
  p->nbin = NBIN;
  const double pi = 3.14159265358979323846;
  for (int n = 0; n < p->wlen; ++n)  // periodic Hann (librosa's default window) / periodic Hamming (torch.hamming_window, :160)
    p->window[n] = mel ? (float)(0.5 - 0.5 * cos(2.0 * pi * n / FN)) : (float)(0.54 - 0.46 * cos(2.0 * pi * n / 320.0));
  for (int n = 0; n < 256; ++n) {
    p->tw256[2 * n] = (float)cos(2.0 * pi * n / 256.0);
    p->tw256[2 * n + 1] = (float)(-sin(2.0 * pi * n / 256.0));
  }
  for (int q = 0; q < 16; ++q) {
    p->tw512[2 * q] = (float)cos(2.0 * pi * q / 512.0);
    p->tw512[2 * q + 1] = (float)(-sin(2.0 * pi * q / 512.0));
  }
  if (!mel) return AIR_OK;
  // librosa.filters.mel(sr=16000, n_fft=512, n_mels=128, fmin=0, fmax=8000, htk=False, norm='slaney') in fp64:
  // fftfreqs = linspace(0, 8000, 257), mel_f = mel_to_hz(linspace(0, hz_to_mel(8000), 130))
  double mel_f[NMEL + 2];
  const double mel_max = hz_to_mel(8000.0);
  for (int i = 0; i < NMEL + 2; ++i) mel_f[i] = mel_to_hz(i == NMEL + 1 ? mel_max : i * (mel_max / (NMEL + 1)));
  int maxw = 1;
  for (int j = 0; j < NMEL; ++j) {
    double w[NBIN];
    int first = -1, last = -1;
    for (int k = 0; k < NBIN; ++k) {
      const double fk = k * (8000.0 / 256.0);
      const double lower = (fk - mel_f[j]) / (mel_f[j + 1] - mel_f[j]);
      const double upper = (mel_f[j + 2] - fk) / (mel_f[j + 2] - mel_f[j + 1]);
      const double tri = fmax(0.0, fmin(lower, upper));
      w[k] = tri * (2.0 / (mel_f[j + 2] - mel_f[j]));  // Slaney: unit area per band
      if (w[k] != 0.0) {
        if (first < 0) first = k;
        last = k;
      }
    }
    if (first < 0) {  // (no filter of this geometry is empty)
      p->lo[j] = 0;
      p->cnt[j] = 0;
      continue;
    }
    const int cnt = last - first + 1;
    if (cnt > MELW || first + MELW > PROW) return AIR_EUNSUPPORTED;  // wider than the banded table / past the padded row
    p->lo[j] = first;
    p->cnt[j] = cnt;
    if (cnt > maxw) maxw = cnt;
    for (int i = 0; i < cnt; ++i) p->fbwT[i * NMEL + j] = (float)w[first + i];
  }
  p->maxw = maxw;
  return AIR_OK;
}

int air_spec_fwd(int kind, const float* pcm, const int16_t* pcm16, int B, int L, float* out, const void* plan_dev,
                 int flags, air_stream_t stream) {
  if ((pcm != nullptr) == (pcm16 != nullptr) || !out || !plan_dev || B <= 0 || L <= 0) return AIR_EINVAL;
  const short* p16 = reinterpret_cast<const short*>(pcm16);
  if (kind == AIR_SPEC_STFT)
    return spec_launch<AIR_SPEC_STFT>(pcm, p16, B, L, nullptr, out, 0, nullptr, plan_dev, spec_flags(kind, flags),
                                      AIR_PAD_REPEAT, false, air_stream(stream));
  if (kind == AIR_SPEC_MEL)
    return spec_launch<AIR_SPEC_MEL>(pcm, p16, B, L, nullptr, out, 0, nullptr, plan_dev, spec_flags(kind, flags),
                                     AIR_PAD_REPEAT, false, air_stream(stream));
  return AIR_EUNSUPPORTED;
}

int air_spec_fwd_ragged(int kind, const float* pcm, const int16_t* pcm16, int B, int Lcap, const int* lengths_dev,
                        float* out, int feat_len, const int* start_dev, const void* plan_dev, int flags, int pad_mode,
                        air_stream_t stream) {
  if ((pcm != nullptr) == (pcm16 != nullptr) || !out || !plan_dev || B <= 0 || Lcap <= 0 || feat_len <= 0)
    return AIR_EINVAL;
  if (pad_mode == AIR_PAD_SILENCE) return AIR_EUNSUPPORTED;  // the silence frame is an LFCC frame (dataset.py:13-16)
  if (pad_mode != AIR_PAD_REPEAT && pad_mode != AIR_PAD_ZERO) return AIR_EINVAL;
  const short* p16 = reinterpret_cast<const short*>(pcm16);
  if (kind == AIR_SPEC_STFT)
    return spec_launch<AIR_SPEC_STFT>(pcm, p16, B, Lcap, lengths_dev, out, feat_len, start_dev, plan_dev,
                                      spec_flags(kind, flags), pad_mode, true, air_stream(stream));
  if (kind == AIR_SPEC_MEL)
    return spec_launch<AIR_SPEC_MEL>(pcm, p16, B, Lcap, lengths_dev, out, feat_len, start_dev, plan_dev,
                                     spec_flags(kind, flags), pad_mode, true, air_stream(stream));
  return AIR_EUNSUPPORTED;
}

}  // extern "C"
