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
// complex FFT on the even/odd packing, done as 16 x 16 with the radix-16 butterfly of air_fft16.h.  The PCM staging, the
// transpose through a padded wave-private LDS tile, the real-FFT untangle against lane (16 - g) of the same 16-lane
// group, the ragged row geometry and both copy-outs are the pieces of air_spec512.h, shared with the LFCC kernel; the
// window (read from the plan at use), the tile overlay and the mel filterbank are this file's own.  The STFT window sits
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
#include "air_spec512.h"

namespace {

constexpr int FN = 512;
constexpr int NBIN = FN / 2 + 1;      // 257
constexpr int NW = 8;                 // waves per workgroup
constexpr int NTHREADS = NW * 64;
constexpr int FT = 4 * NW;            // 32 frames computed and written per workgroup
constexpr int PROW = 264;             // MEL: power-spectrum row stride; zeros behind the Nyquist bin
constexpr int XCH_FLOATS = 4 * 16 * SPEC512_XROW;  // wave-private: the 4 x 16 x 17 transposition, then (MEL) 4 power rows
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
    const Spec512Row r = spec512_row<HOP, FT, true>(a.lengths, a.start, b, a.L, a.feat_len, t0);
    if (r.dead) return;  // (workgroup-uniform, ahead of every barrier and of the staging)
    L = r.L;
    T = r.T;
    live_tiles = r.live_tiles;
  }
  const float* __restrict__ row = a.pcm ? a.pcm + (size_t)b * a.L : nullptr;
  const short* __restrict__ row16 = a.pcm16 ? a.pcm16 + (size_t)b * a.L : nullptr;

  // ---- stage the filter weights and the PCM --------------------------------
  if constexpr (MEL) {
    for (int e = tid; e < MELW * NMEL; e += NTHREADS) s_fbw[e] = plan->fbwT[e];
  }
  const long s0 = (long)HOP * t0 - G::LEAD;  // first staged sample (may be < 0); a multiple of 4
  spec512_stage<NSAMP, NTHREADS, MEL>(row, row16, L, s0, !MEL && (a.flags & FLAG_EMPH) != 0,
                                      MEL && (a.flags & FLAG_REFLECT) != 0, s_main, tid);

  // ---- per-lane constants --------------------------------------------------
  const int f = lane >> 4;       // frame within the wave's 4-frame group
  const int g = lane & 15;       // lane within the frame
  const int fi = wave * 4 + f;   // frame within the tile
  const bool active = t0 + wave * 4 < T;  // wave-uniform: the group holds a frame of the row
  const Spec512Lane ln = spec512_lane(plan->tw512, lane);
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
    spec512_transpose_fft(x, xch, f, g);  // Z[g + 16 p] = x[p]; MEL: the exchange tile is reused for the power rows below

    // where bin k of this lane's frame goes: the output tile (STFT) or the wave's power row (MEL)
    auto put = [&](int k, float pw) {
      if constexpr (MEL) xch[f * PROW + k] = pw;
      else if constexpr (PADDED) s_out[k * OSTR + fi] = pw;
      else s_out[fi * D + k] = pw;
    };
#pragma unroll
    for (int p = 0; p < 16; ++p) put(g + 16 * p, spec512_bin_power(x, p, g, ln));
    if (g == 0) put(256, spec512_nyquist_power(x));

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
    spec512_store_dense<NTHREADS>(orow, s_out, min(FT, T - t0) * D, D, tid);
  } else {
    // (a 32-lane run of the copy-out is one bin's 32 frames)
    spec512_store_padded<FT, NTHREADS, false>(a.out + (size_t)b * D * a.feat_len, s_out, D, T, t0, tile, live_tiles,
                                              a.feat_len, a.start, b, a.pad_mode, nullptr, tid);
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
  if (mel) {
    for (int n = 0; n < FN; ++n) p->window[n] = (float)(0.5 - 0.5 * cos(2.0 * SPEC512_PI * n / FN));  // periodic Hann (librosa's default)
  } else {
    spec512_fill_hamming(p->window, 320);  // torch.hamming_window (:160); taps 320 .. 511 stay zero
  }
  spec512_fill_twiddles(p->tw256, p->tw512);
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
