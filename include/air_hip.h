/* air_hip.h -- C-ABI of the MI355X (gfx950) hot path of ASVspoof2021_AIR.
 *
 * The reference (yzyouzhang/ASVspoof2021_AIR) is pure Python/PyTorch and has no
 * FFI; the boundary it exposes for this path is the Python module surface
 * (SURVEY.md §8b).  This header is the C-ABI a binding for that surface calls:
 * each entry point names the reference function (file:line) whose device work
 * it replaces.  Conventions:
 *   - plain pointers and sizes only; device pointers unless suffixed _host
 *   - no allocation inside: callers pass workspaces (see *_ws_bytes queries)
 *   - every launch goes to the caller's stream (air_stream_t == hipStream_t)
 *   - return 0 (AIR_OK) or a negative AIR_E* code; never throws
 *   - no per-call global state; re-entrant across streams.  The only process-wide
 *     state is the dispatch-option table below (air_set_option): which of several
 *     equivalent kernels serves a call
 *   - tensors are contiguous fp32, NCHW / (B,C,T) / (B,T,D) as stated per call
 */
#ifndef AIR_HIP_H
#define AIR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* air_stream_t; /* hipStream_t */

#define AIR_OK 0
#define AIR_EINVAL (-1)       /* bad argument (null pointer, non-positive size) */
#define AIR_EUNSUPPORTED (-2) /* valid request this build has no kernel for */
#define AIR_ELAUNCH (-3)      /* HIP reported a launch error */
#define AIR_EWORKSPACE (-4)   /* workspace too small */

/* Library identification: returns "air_hip gfx950 <abi-version>". */
const char* air_version(void);
int air_abi_version(void);

/* ------------------------------------------------------- dispatch options --
 * Process-wide switches between equivalent kernels (A/B measurement, and the
 * strict-parity configuration of the tests).  Each option NAME is seeded once
 * from the environment variable AIR_<NAME>; air_set_option changes it at run
 * time (takes effect at the next call; not meant to be flipped while another
 * thread is launching).  Unknown names return AIR_EINVAL.
 *   NO_WINO4 (0)          1: 3x3/stride-1 forward+dgrad skip Winograd F(4x4,3x3)
 *   NO_WINOGRAD (0)       bit 1: 3x3/stride-1 forward+dgrad on the direct f32-MFMA
 *                         kernels; bit 2: weight gradients too.  3 = every
 *                         convolution is an fmaf chain (round-1 tolerances hold)
 *   WINO4_SPLIT (1)       0 never / 1 when the last round is > 13 % empty / 2 always:
 *                         cut the Winograd k-step stream evenly over the workgroups
 *   WINO4_TH3 (2)         0: F(4x4,3x3) tiles always; 1: F(3x4,3x3) where it issues fewer
 *                         positions for the image height (H = 9, 5, 3); 2: also on ties (H = 18)
 *   WINO4_XCD (2)         0: work items dealt round-robin over the whole chip; 1: an XCD owns a
 *                         contiguous range of the item list; 2: an XCD owns the tile quads
 *                         congruent to its index (same L2 sharing as 1, measured faster)
 *   CONV_MT (0)           force the direct kernels' pixel-tile count (1 | 2)
 *   WGRAD_WGS (256), WINO_WGRAD_WGS (256)   workgroups of the split-K weight gradients
 *   DIRECT_WGRAD_ROWS (1) row-staged conv1 weight gradient
 *   C1B_PS (7)            bit mask of the persistent bf16 pointwise kernels
 *   C1B_GEMM_PS (1)       256x256 persistent bf16 GEMM
 *   SKINNY_WGRAD (1)      streaming weight gradient of the 16 -> 64 1x1 layer (0: generic 64-channel tiles)
 *   WINO4_DEPHASE (0)     every second persistent Winograd workgroup starts N x 4096 cycles late, so that the store
 *                         sections of neighbouring workgroups do not coincide (measured: profiles/r05_wino4_dephase.md)
 *   CONV_S2 (31)          bit 1: stride-2 forward in 4-channel (3x3) / 16-channel (1x1) K chunks (three resident
 *                         workgroups per CU instead of one; same arithmetic, chunk boundaries only); bit 2: stride-2
 *                         3x3 data gradient in one pass; bit 4: stride-2 3x3 forward on the bf16 matrix cores as six
 *                         bf16 products per fp32 product (operands split exactly into three bf16 planes: fp32-
 *                         equivalent arithmetic, csrc/conv_bf3.hip); bit 8: the same for the paired stride-2 data
 *                         gradient (air_conv2d_dgrad_s2_pair); bit 16: the stride-2 3x3 weight gradient likewise
 *   TAP_ROWS (0)          the 64 -> 64 Res2 convs on bf16-resident rows (air_h_conv1d_tap*) stage their operand as 16-byte
 *                         row pieces (8 frames of a channel, transposed into LDS) instead of 2-byte loads down the
 *                         channels; same sums in the same order (air_h_conv1d_tap_pro always does; measured -0.7 % of
 *                         the ECAPA step without a prologue: off)
 *   RESAMPLE_TABLE_LDS (1) air_resample_ragged / air_wav_decode copy a rate's coefficient table into LDS when it fits
 *                         (8 / 24 / 32 / 48 kHz -> 16 kHz); 0: every table is read through L2.  Same sums, same order.
 */
int air_set_option(const char* name, int value);
int air_get_option(const char* name, int* value_out);
int air_option_count(void);
const char* air_option_name(int index); /* NULL when out of range */

/* Compute units a launch on `stream` can occupy: the stream's CU mask (hipExtStreamCreateWithCUMask, or the
 * process-wide ROC_GLOBAL_CU_MASK) capped by the device's CU count.  The persistent kernels (one workgroup per
 * CU: the Winograd convolutions) size their grids by it, and wino4_conv_kernel cuts tail items between two
 * workgroups only when every workgroup of the launch is resident at once.  No reference counterpart
 * (main_train.py:101 pins one whole GPU through CUDA_VISIBLE_DEVICES). */
int air_stream_compute_units(air_stream_t stream);

/* ------------------------------------------------------------------ LFCC --
 * Replaces LFCC.forward (feature_extraction.py:93-138) incl. delta (:41-58),
 * with the filterbank of LFCC.__init__ (:77-86) and the LinearDCT weight
 * (utils_dsp.py:233-244) folded into a small "plan" blob built on the host.
 */
size_t air_lfcc_plan_bytes(void);
/* fb_host: [nbin][nfilt] row-major (module.lfcc_fb); dct_host: [nfilt][nfilt]
 * (module.l_dct.weight, y = x @ W^T); window_host: [fl] analysis window
 * (torch.hamming_window(fl), :110) or NULL for the periodic Hamming closed form.
 * fl/fs/fn = window / hop / FFT length (this build: 320/160/512, nfilt <= 32).
 * Writes air_lfcc_plan_bytes() bytes to plan_host_out; the caller uploads it. */
int air_lfcc_plan_build(const float* fb_host, int nbin, int nfilt, const float* dct_host,
                        const float* window_host, int fl, int fs, int fn, void* plan_host_out);
#define AIR_LFCC_EMPHASIS 1 /* pre-emphasis 0.97 (feature_extraction.py:105-106) */
#define AIR_LFCC_DELTA 2    /* append delta and delta-delta (:130-133) */
/* pcm: (B, L) fp32, NOT modified.  out: (B, 1 + L/fs, nfilt * (3 if DELTA else 1)). */
int air_lfcc_fwd(const float* pcm, int B, int L, float* out, const void* plan_dev, int flags,
                 air_stream_t stream);
/* Fused variant writing the model-input layout the trainer builds on the host
 * (dataset.py:66-79 pad/chop + main_train.py:338 transpose): out is
 * (B, D, feat_len) with frame t' taken from frame (start[b] + t') mod T when
 * T < feat_len ("repeat" padding, dataset.py:519-522) or start[b] + t' when
 * T >= feat_len (chop; start_dev may be NULL = 0).  */
int air_lfcc_fwd_padded(const float* pcm, int B, int L, float* out, int feat_len,
                        const int* start_dev, const void* plan_dev, int flags, air_stream_t stream);
/* All three pad modes of the reference's --padding flag (main_train.py:45, dataset.py:72-79) for inputs
 * shorter than feat_len; longer inputs are chopped at start[b] (clamped to [0, T - feat_len]) whatever the mode:
 *   AIR_PAD_REPEAT  tile the frames (dataset.py:519-522)
 *   AIR_PAD_ZERO    append zero frames (dataset.py:513-517)
 *   AIR_PAD_SILENCE PREPEND silence_dev (D floats: the LFCC frame of digital silence, dataset.py:13-16, :524-528)
 * Exactly one of pcm (fp32) / pcm16 (16-bit PCM) is non-NULL.  Any other pad_mode: AIR_EINVAL (the reference
 * raises ValueError, dataset.py:79). */
#define AIR_PAD_REPEAT 0
#define AIR_PAD_ZERO 1
#define AIR_PAD_SILENCE 2
int air_lfcc_fwd_padded_ex(const float* pcm, const int16_t* pcm16, int B, int L, float* out, int feat_len,
                           const int* start_dev, const void* plan_dev, int flags, int pad_mode,
                           const float* silence_dev, air_stream_t stream);
/* Ragged batch: B rows of capacity Lcap (row b = pcm + b * Lcap), of which the first lengths_dev[b] samples are the
 * utterance.  Row b of out, (B, D, feat_len), is exactly what air_lfcc_fwd_padded_ex writes for that utterance alone
 * with L = L_b = clamp(lengths_dev[b], 1, Lcap) (the clamp only keeps a bad device value inside its row): same crop
 * clamp, pad modes and deltas clamped at the utterance's own ends.  No sample at index >= L_b is read.  One launch of
 * B x ceil((1 + Lcap/fs) / 28) workgroups; those a row does not need return at once.  Exactly one of pcm / pcm16 is
 * non-NULL; feat_len <= 0, a NULL lengths_dev or a bad pad_mode: AIR_EINVAL. */
int air_lfcc_fwd_ragged(const float* pcm, const int16_t* pcm16, int B, int Lcap, const int* lengths_dev, float* out,
                        int feat_len, const int* start_dev, const void* plan_dev, int flags, int pad_mode,
                        const float* silence_dev, air_stream_t stream);
/* Same from 16-bit PCM as stored in the corpus' wav/flac files: the kernel converts s -> s / 32768 (exact, what
 * soundfile/librosa hand the reference, preprocess.py:239-241), so the features are bit-identical to the fp32
 * entry points on the converted samples while the kernel reads half the bytes (128 KB instead of 256 KB per
 * 4 s utterance) and the caller uploads half as much.  feat_len <= 0 selects the (B, T, D) layout. */
int air_lfcc_fwd_padded_i16(const int16_t* pcm16, int B, int L, float* out, int feat_len,
                            const int* start_dev, const void* plan_dev, int flags, air_stream_t stream);
/* The reference mutates its input (feature_extraction.py:106).  This applies
 * the same in-place x[n] -= coef*x[n-1] (n>=1).  ws: >= air_preemph_ws_bytes. */
size_t air_preemph_ws_bytes(int B, int L);
int air_preemph_inplace(float* pcm, int B, int L, float coef, void* ws, size_t ws_bytes,
                        air_stream_t stream);
/* (B,T,D) -> (B,D,feat_len) repeat-pad / chop + transpose (dataset.py:66-79, main_train.py:338). */
int air_pad_transpose(const float* feat, int B, int T, int D, float* out, int feat_len,
                      const int* start_dev, air_stream_t stream);
/* ... with the pad mode of air_lfcc_fwd_padded_ex (dataset.py:513-528). */
int air_pad_transpose_ex(const float* feat, int B, int T, int D, float* out, int feat_len,
                         const int* start_dev, int pad_mode, const float* silence_dev, air_stream_t stream);

/* ---------------------------------------------------- STFT and Melspec --
 * The reference's two other front-ends, each one launch from PCM (csrc/spectral.hip):
 *   AIR_SPEC_STFT  replaces STFT.forward (feature_extraction.py:154-165; dumped by preprocess.py:35-47): optional
 *                  pre-emphasis 0.97 (:157), torch.stft(x, 512, 160, 320, hamming_window(320), pad_mode="constant")
 *                  (:159-161), norm(., 2, -1).pow(2) (:163).  T = 1 + L / 160, D = 257, no log.
 *   AIR_SPEC_MEL   replaces Melspec.forward (feature_extraction.py:174-176; preprocess.py:176-215, :247-258):
 *                  librosa.feature.melspectrogram(sr=16000, n_fft=512, hop_length=128) - periodic Hann window of 512,
 *                  centred frames with 256 reflected (AIR_SPEC_REFLECT) or zero samples each side, power 2.0, the
 *                  128-band Slaney mel filterbank with Slaney normalisation.  T = 1 + L / 128, D = 128, no log.
 * These are the only geometries.  The plan blob (built on the host, uploaded by the caller) is
 *   int32[8]  kind, D, hop, window length, 257, widest mel filter, 0, 0
 *   float[512] window (STFT: 320 taps, then zeros)   float[512] + float[32] FFT twiddles
 *   int32[128] first bin of mel filter j             int32[128] bins it spans
 *   float[12][128] weight of bin first[j] + i in filter j, fp64 formulas rounded once (zero for STFT). */
#define AIR_SPEC_STFT 1
#define AIR_SPEC_MEL 2
#define AIR_SPEC_EMPHASIS 1 /* STFT: pre-emphasis 0.97 on the original samples (feature_extraction.py:157) */
#define AIR_SPEC_REFLECT 2  /* MEL: pad_mode "reflect" (librosa's default before 0.10); unset: "constant" */
size_t air_spec_plan_bytes(void);
int air_spec_plan_build(int kind, void* plan_host_out);
/* D of a kind: 257 / 128 (AIR_EINVAL for anything else). */
int air_spec_out_dim(int kind);
/* Exactly one of pcm (B, L) fp32 / pcm16 (16-bit PCM, x = s / 32768) is non-NULL; neither is modified.
 * out: (B, 1 + L / hop, D).  A plan of the other kind: nothing is written. */
int air_spec_fwd(int kind, const float* pcm, const int16_t* pcm16, int B, int L, float* out, const void* plan_dev,
                 int flags, air_stream_t stream);
/* The model-input layout (dataset.py:62-79 pad / chop + main_train.py:338 transpose): out is (B, D, feat_len).  Row b
 * holds L_b = clamp(lengths_dev[b], 1, Lcap) samples (lengths_dev NULL: every row holds Lcap); no sample at index
 * >= L_b is read.  T_b > feat_len: chopped at start_dev[b], clamped to [0, T_b - feat_len] (NULL = 0); T_b < feat_len:
 * AIR_PAD_REPEAT tiles the frames (dataset.py:519-522), AIR_PAD_ZERO appends zero frames (:513-517).
 * AIR_PAD_SILENCE: AIR_EUNSUPPORTED - the reference's silence frame is an LFCC frame (dataset.py:13-16).  Under
 * AIR_SPEC_REFLECT a row shorter than 257 samples has no reflection to read (numpy raises); its indices are clamped
 * into the row.  One launch of B x ceil((1 + Lcap / hop) / 32) workgroups; those a row does not need return at once. */
int air_spec_fwd_ragged(int kind, const float* pcm, const int16_t* pcm16, int B, int Lcap, const int* lengths_dev,
                        float* out, int feat_len, const int* start_dev, const void* plan_dev, int flags, int pad_mode,
                        air_stream_t stream);

/* ------------------------------------------------------- CQCC front-end --
 * Constant-Q cepstral coefficients, the reference's second feature (--feat CQCC).  The reference ships no CQCC code,
 * so the feature is DEFINED by these formulas (csrc/cqcc.hip; tests/cqcc_oracle.py restates them in numpy fp64);
 * parity with the challenge's MATLAB toolbox is not claimed.
 *
 *   sr 16000, B = bins_per_octave 96, O = n_octaves 9, hop 160, n_coef 20 (c0 included), d 16, eps 2^-52.
 *   fmax = sr / 2, fmin = fmax / 2^O, K = B O bins at f_k = fmin 2^(k / B); Q = 1 / (2^(1/B) - 1).
 *   Octave o = O - 1 - k / B (integer division); o = 0 is the top one.
 *
 *   1. Pyramid.  Level 0 is the row (16-bit PCM as s / 32768, no pre-emphasis), L_0 = L samples.  Level s + 1 has
 *      L_{s+1} = ceil(L_s / 2) samples, x_{s+1}[n] = sum_j h[j] x_s[2 n + j - (J - 1) / 2], zeros outside [0, L_s).
 *      h: J = 47 taps, h[j] = 0.5 sinc((j - 23) / 2) kaiser_47(beta = 16)[j], scaled to unit sum: a half-band low-pass
 *      whose stopband from 3 R / 8 is below -150 dB (the oracle's test measures it), i.e. below fp32 roundoff.
 *      Octaves 0 and 1 are analysed at level 0, octave o >= 2 at level o - 1: every band but the top one lies in
 *      [R/8, R/4) of its own rate R, where h is flat and what folds onto it comes from beyond 3 R / 8.
 *   2. Atoms.  At rate R the bin at f has N = 2 floor(Q R / (2 f)) + 1 samples, a symmetric Hann window w over them
 *      (w[n] = 0.5 - 0.5 cos(2 pi n / (N - 1))), and
 *        X[k, t] = (1 / sum w) sum_n w[n] x_s[c + n - (N-1)/2] exp(-2 pi i f (n - (N-1)/2) / R),  c = floor(t hop / 2^s),
 *      zeros outside the level.  In f / R the atoms of all octaves >= 1 are one table (N = 555 .. 1103), the top
 *      octave's a second (N = 277 .. 551); both are formed in fp64 and rounded once.
 *   3. Frames.  T_b = 1 + L_b / hop.
 *   4. S[k, t] = log(|X|^2 + eps).
 *   5. S is read by linear interpolation in k at B log2(g_m / fmin), g_m = fmin (1 + m / d), m < M = 1 + floor(d
 *      (f_{K-1} / fmin - 1)) (8118 at the defaults); the orthonormal DCT-II of those M values gives c_q, q < n_coef.
 *      The plan holds the product of both steps, one (n_coef x K) matrix formed in fp64.
 *   6. Delta and delta-delta as in the LFCC front-end (x[t + 1] - x[t - 1] with the edge frames repeated, twice), over
 *      the row's own frames.  Columns [static, delta, delta-delta], D = 3 n_coef.
 *
 * Built: bins_per_octave 96, n_octaves 1 .. 9, hop 1 .. 160, n_coef 1 .. 32 (anything else: AIR_EUNSUPPORTED).  The
 * plan blob (air_cqcc_plan_bytes() bytes, built on the host, uploaded by the caller): int32[12] tag, O, hop, n_coef, K,
 * J, half-lengths of the two tables, d, M, 0, 0; float[4] eps, 0, 0, 0; float[64] h; float[32][864] P (rows of K
 * floats, packed); float[576][192] and float[1120][192] atom tables, row = tap, column 32 (bin / 16) + 16 part + bin % 16
 * with part 0 = real, 1 = imaginary.  n_octaves, hop and n_coef travel as arguments too (they size the launches); a
 * plan that disagrees with them writes nothing. */
size_t air_cqcc_plan_bytes(void);
int air_cqcc_plan_build(int bins_per_octave, int n_octaves, int hop, int n_coef, int d, double eps,
                        void* plan_host_out);
/* K = bins_per_octave * n_octaves (AIR_EUNSUPPORTED outside what is built). */
int air_cqcc_n_bins(int bins_per_octave, int n_octaves);
/* Scratch of one call, a function of (B, Lcap) and the geometry only: the pyramid levels, the (B, T, K) log spectrum
 * (89 MB at 64 x 64 000 samples) and the (B, T, n_coef) statics.  0 for a geometry that is not built. */
size_t air_cqcc_ws_bytes(int B, int Lcap, int n_octaves, int hop, int n_coef);
/* Exactly one of pcm (B, L) fp32 / pcm16 is non-NULL; neither is modified.  out: (B, 1 + L / hop, 3 n_coef).  No host
 * synchronisation; every sum in a fixed order, no atomics. */
int air_cqcc_fwd(const float* pcm, const int16_t* pcm16, int B, int L, float* out, const void* plan_dev,
                 int n_octaves, int hop, int n_coef, void* ws, size_t ws_bytes, air_stream_t stream);
/* Rows of L_b = clamp(lengths_dev[b], 1, Lcap) samples (NULL: Lcap); no sample at index >= L_b is read, and row b is,
 * bit for bit, what the dense call gives for it alone.  feat_len <= 0: out is (B, 1 + Lcap / hop, 3 n_coef) and only
 * the first T_b frames of row b are written; otherwise out is (B, 3 n_coef, feat_len), padded / chopped as in
 * air_spec_fwd_ragged (AIR_PAD_REPEAT, AIR_PAD_ZERO; AIR_PAD_SILENCE: AIR_EUNSUPPORTED). */
int air_cqcc_fwd_ragged(const float* pcm, const int16_t* pcm16, int B, int Lcap, const int* lengths_dev, float* out,
                        int feat_len, const int* start_dev, const void* plan_dev, int n_octaves, int hop, int n_coef,
                        int pad_mode, void* ws, size_t ws_bytes, air_stream_t stream);
/* Step 4 alone: out is (B, 1 + Lcap / hop, K), the first T_b frames of row b written (lengths_dev may be NULL). */
int air_cqcc_spectrum(const float* pcm, const int16_t* pcm16, int B, int Lcap, const int* lengths_dev, float* out,
                      const void* plan_dev, int n_octaves, int hop, int n_coef, void* ws, size_t ws_bytes,
                      air_stream_t stream);

/* --------------------------------------------------------------- conv2d --
 * Replaces nn.Conv2d forward/backward as used by resnet.py:131,56-61,140
 * (bias=False everywhere).  NCHW fp32.  Implicit GEMM on f32 MFMA.
 * Optional fused prologue: per-input-channel y = max(0, x*scale[c]+shift[c])
 * (BatchNorm apply + ReLU of the pre-activation block, resnet.py:64,67)
 * applied while staging the input; optional epilogue residual add
 * (resnet.py:68).  3x3 / stride 1 / pad 1 layers without the fused prologue run
 * as Winograd F(4x4,3x3) (forward, dgrad: csrc/conv_wino4.hip) and F(3x3,2x2)
 * (wgrad: csrc/conv_wino.hip); results within 2e-5 of the output scale of the
 * fp64 convolution (direct kernels: 3e-6).
 */
typedef struct AirConv2d {
  int B, Cin, H, W;       /* input */
  int Cout, KH, KW;       /* filter */
  int sh, sw, ph, pw;     /* stride, zero padding */
  int Ho, Wo;             /* output (must equal the conv arithmetic) */
} AirConv2d;

size_t air_conv2d_ws_bytes(const AirConv2d* p);
/* y = conv(act(x), w) [+ residual].  in_scale/in_shift NULL = identity prologue.
 * relu: apply max(0,.) after the affine prologue.
 * stats: NULL, or a 16-byte aligned buffer of air_conv2d_fwd_stats_bytes(p) bytes (0 = this layer has no fused
 * statistics under the current dispatch options: pass NULL) that receives BatchNorm statistics of y (of y + residual)
 * from the convolution's epilogue: one record {n, K, sum(y - K), sum((y - K)^2)} per (channel, tile group) of the
 * Winograd F(3x4 / 4x4, 3x3) kernel - the (count, mean, M2) of the group's outputs in shifted form.  Hand the buffer
 * to air_bn_stats as stats_in and the BatchNorm that follows the convolution (resnet.py:63-69: conv1 -> bn2, block
 * output -> the next block's bn1) merges the records in fp64 instead of reading y again: 12 of the 18 statistics
 * passes of a ResNet-18 step.  Round 4, measured (rounds 2 and 3 had priced it and not built it): see DESIGN.md. */
size_t air_conv2d_fwd_stats_bytes(const AirConv2d* p);
int air_conv2d_fwd(const AirConv2d* p, const float* x, const float* w, float* y,
                   const float* in_scale, const float* in_shift, int relu,
                   const float* residual, double* stats, void* ws, size_t ws_bytes,
                   air_stream_t stream);
/* dx = conv_transpose(dy, w) [+ accumulate]: gradient w.r.t. the (activated) conv
 * input.  accumulate: NULL or a tensor shaped like dx that is added (may alias dx;
 * used to join the 1x1-shortcut and 3x3 branches of a PreActBlock). */
int air_conv2d_dgrad(const AirConv2d* p, const float* dy, const float* w, float* dx,
                     const float* accumulate, void* ws, size_t ws_bytes, air_stream_t stream);
/* Weight transforms off the critical path.  The 3x3 / stride 1 / pad 1 layers run as Winograd kernels whose
 * transformed weights (G g G^T, packed) are otherwise produced by a small kernel in front of EVERY forward and dgrad
 * launch (25 + 25 launches of ~9 us per ResNet-18 step, serialised with the convs).  They depend on the weights
 * only: air_conv2d_prepack writes them for `pass` (0 forward, 1 dgrad) into a caller-owned buffer of
 * air_conv2d_prepack_bytes(p, pass) bytes (0 = this layer / pass has no such form) - on any stream, e.g. a side
 * stream at the start of the step - and the _pre entry points take that buffer as w_packed (NULL = transform here).
 * Round 3: the direct kernels' weight slabs (stride-2 3x3, 1x1, conv5, the parity classes of a stride-2 data
 * gradient: 28 more ~5 us launches per step) travel the same way: air_conv2d_prepack writes every slab the pass
 * consumes, in consumption order (one code path walks them for sizing, packing and use).  A buffer must be consumed
 * under the dispatch options it was produced under. */
size_t air_conv2d_prepack_bytes(const AirConv2d* p, int pass);
/* The layout air_conv2d_prepack writes for (p, pass) under the current dispatch options: a binding records it beside the
 * buffer and compares at use (options can change in between; the layouts differ in element type, not only in size). */
enum { AIR_PACK_NONE = 0, AIR_PACK_F32_SLABS = 1, AIR_PACK_WINO2 = 2, AIR_PACK_BF3 = 3, AIR_PACK_WINO4 = 4 };
int air_conv2d_prepack_layout(const AirConv2d* p, int pass);
int air_conv2d_prepack(const AirConv2d* p, const float* w, int pass, void* out, size_t out_bytes,
                       air_stream_t stream);
/* Between _begin and _flush the air_conv2d_prepack / air_conv2d_dgrad_s2_pair_prepack calls of the calling thread only
 * RECORD their transforms; _flush runs them on `stream` as one launch per 32 Winograd transforms and one per 32 direct
 * slabs (a ResNet-18 step: 3 launches for 47).  The output buffers are valid behind _flush in stream order. */
int air_conv2d_prepack_begin(void);
int air_conv2d_prepack_flush(air_stream_t stream);
int air_conv2d_fwd_pre(const AirConv2d* p, const float* x, const float* w, const void* w_packed, float* y,
                       const float* in_scale, const float* in_shift, int relu, const float* residual,
                       double* stats, void* ws, size_t ws_bytes, air_stream_t stream);
int air_conv2d_dgrad_pre(const AirConv2d* p, const float* dy, const float* w, const void* w_packed, float* dx,
                         const float* accumulate, void* ws, size_t ws_bytes, air_stream_t stream);
/* The same data gradient when dx is the gradient with respect to the OUTPUT of relu(batchnorm(bn_x)) - the activated
 * tensor a 3x3 / stride 1 convolution of a PreActBlock reads (resnet.py:63-69: bn2 -> relu -> conv2, and bn1 -> relu
 * -> conv1 in the blocks without a 1x1 shortcut).  The epilogue that writes dx also takes the two per-channel sums the
 * BatchNorm backward needs - sum g and sum g * xhat with g = dx where bn_x * scale + shift > 0, xhat = (bn_x - mean) *
 * invstd, the arithmetic of air_bn_bwd's own first pass - into `sums` (air_conv2d_dgrad_bn_sums_bytes(p) bytes,
 * 16-byte aligned; 0 = this layer has no such form under the current dispatch options: call air_conv2d_dgrad_pre).
 * Hand `sums` to air_bn_bwd_ex3 and the BatchNorm backward skips the pass that re-reads dx and bn_x (12 of the 18
 * BatchNorm backward passes of a ResNet-18 step).  bn_x has dx's shape; the four vectors have Cin entries. */
size_t air_conv2d_dgrad_bn_sums_bytes(const AirConv2d* p);
int air_conv2d_dgrad_bn(const AirConv2d* p, const float* dy, const float* w, const void* w_packed, float* dx,
                        const float* accumulate, const float* bn_x, const float* bn_mean, const float* bn_invstd,
                        const float* bn_gamma, const float* bn_beta, void* sums, void* ws, size_t ws_bytes,
                        air_stream_t stream);
/* Forward of the two convolutions a stride-2 PreActBlock applies to the SAME activated input (resnet.py:56 conv1 3x3 /
 * stride 2 / pad 1 and :61-66 the 1x1 / stride 2 shortcut, both reading `out` of :64) in one launch (round 5, split-bf16
 * kernel of csrc/conv_bf3.hip: the shortcut's operand is the centre tap's fragment, already loaded and split): y =
 * conv1(x), y_sc = shortcut(x).  p describes the 3x3 layer.  _prepack_bytes 0 / AIR_EUNSUPPORTED: not this shape, or
 * option CONV_S2 bit 4 off - a binding then makes the two air_conv2d_fwd calls.  packed: the buffer _prepack wrote under
 * the same options, or NULL (then ws, >= _prepack_bytes, receives the planes in front of the launch). */
size_t air_conv2d_fwd_s2_pair_prepack_bytes(const AirConv2d* p);
int air_conv2d_fwd_s2_pair_prepack(const AirConv2d* p, const float* w, const float* w_sc, void* out, size_t out_bytes,
                                   air_stream_t stream);
int air_conv2d_fwd_s2_pair(const AirConv2d* p, const float* x, const float* w, const float* w_sc, const void* packed,
                           float* y, float* y_sc, void* ws, size_t ws_bytes, air_stream_t stream);

/* The data gradient of a PreActBlock's stride-2 pair in one pass (resnet.py:56-66: conv1 3x3 / stride 2 / pad 1 and
 * the 1x1 / stride 2 shortcut read the same activated tensor): dx = conv_transpose(dy, w) + conv_transpose(dy_sc, w_sc)
 * [+ accumulate].  p describes the 3x3 convolution; the shortcut has its Cin, Cout, input and output shape.  A wave
 * keeps all four parity classes of its dx tile in registers, so dy is read once and dx leaves as whole rows (rounds 1-3:
 * four class launches + a read-modify-write launch for the shortcut).  `packed`: NULL (the weights are packed into ws,
 * air_conv2d_dgrad_s2_pair_prepack_bytes(p) bytes, in front of the launch) or the buffer air_conv2d_dgrad_s2_pair_prepack
 * wrote under the same dispatch options.  _prepack_bytes 0 / AIR_EUNSUPPORTED: not this shape, or option CONV_S2 bit 2
 * is off - call air_conv2d_dgrad twice.  air_conv2d_dgrad itself takes the same kernel for a lone 3x3 / stride 2. */
size_t air_conv2d_dgrad_s2_pair_prepack_bytes(const AirConv2d* p);
int air_conv2d_dgrad_s2_pair_prepack(const AirConv2d* p, const float* w, const float* w_sc, void* out, size_t out_bytes,
                                     air_stream_t stream);
int air_conv2d_dgrad_s2_pair(const AirConv2d* p, const float* dy, const float* w, const float* dy_sc, const float* w_sc,
                             const void* packed, float* dx, const float* accumulate, void* ws, size_t ws_bytes,
                             air_stream_t stream);
/* dw = correlation(act(x), dy); same prologue as fwd so the activated tensor
 * is never materialised. */
int air_conv2d_wgrad(const AirConv2d* p, const float* x, const float* dy, float* dw,
                     const float* in_scale, const float* in_shift, int relu,
                     void* ws, size_t ws_bytes, air_stream_t stream);

/* ------------------------------------------- adversarial channel head ----
 * model.ChannelClassifier (model.py:976-1023: GRL -> Linear -> Dropout(0.3) -> ReLU -> Linear ->
 * ReLU) and nn.CrossEntropyLoss (main_train.py:251) of the --ADV_AUG branch
 * (main_train.py:377-403, :420-453).  The two Linear layers use air_linear_fwd / air_linear_bwd. */
/* keep[i] = (u_i >= p) / (1 - p), u from Philox4x32-10(seed, offset + i/4): nn.Dropout's scaled mask. */
int air_dropout_mask(float* keep, size_t n, float p, uint64_t seed, uint64_t offset, air_stream_t stream);
/* y = relu(x * keep); keep NULL = eval mode. */
int air_mask_relu_fwd(const float* x, const float* keep, size_t n, float* y, air_stream_t stream);
/* dx = alpha * dy * keep * (y > 0). */
int air_mask_relu_bwd(const float* dy, const float* y, const float* keep, size_t n, float alpha, float* dx,
                      air_stream_t stream);
/* x *= alpha (gradient reversal: alpha = -lambda, model.py:990-995). */
int air_scale(float* x, size_t n, float alpha, air_stream_t stream);
/* probs = softmax(logits (B,C)); loss = mean_b -log probs[b][labels[b]]; *correct = #(argmax == label). */
int air_softmax_ce_fwd(const float* logits, const long long* labels, int B, int C, float* probs, float* loss,
                       int* correct_or_null, air_stream_t stream);
/* dlogits = g * (probs - onehot(labels)) / B, g = *gscale_or_null (device scalar) or 1. */
int air_softmax_ce_bwd(const float* probs, const long long* labels, int B, int C, const float* gscale_or_null,
                       float* dlogits, air_stream_t stream);

/* ------------------------------------------------- channel augmentation --
 * On-the-fly IR convolution ahead of the LFCC kernel (BASELINE.json configs[4]).  Replaces the
 * OFFLINE augmentation of channel_simulation/simulated_device.py:16-61 and
 * simulated_device_channel.py:6-56, which shell out to the un-vendored idiap/acoustic-simulator
 * tool (PARITY UNPINNED: spec = oracle/channel.py, checked against scipy.signal.fftconvolve).
 * y[b] = (x[b] * irs[ir_idx[b]])[:L]; ir_idx[b] < 0 copies the utterance unchanged; ir_idx NULL
 * uses IR 0 for all.  normalize != 0 rescales each augmented utterance to its input peak
 * (max|y| = max|x|).  irs is (n_ir, H) fp32, rows zero-padded to H taps.  x and y must not alias. */
size_t air_ir_convolve_ws_bytes(int B);
/* Round 5: with a workspace of air_ir_convolve_ws_bytes_ex(B, n_ir, H) bytes (>= the above), impulse responses of
 * 128 .. 1025 taps are convolved by overlap-save FFT (option IR_FFT, default 1; same result to fp32 FFT rounding, ~10 x
 * faster at 1024 taps); with the smaller workspace, or any other H, the direct FIR runs. */
size_t air_ir_convolve_ws_bytes_ex(int B, int n_ir, int H);
int air_ir_convolve(const float* x, int B, int L, const float* irs, int n_ir, int H, const int* ir_idx,
                    int normalize, float* y, void* ws, size_t ws_bytes, air_stream_t stream);
/* Ragged batch: B rows of capacity Lcap (row b = x + b * Lcap), of which the first L_b = clamp(lengths_dev[b], 1, Lcap)
 * samples are the utterance (the clamp only keeps a bad device value inside its row).  Exactly one of x (fp32) / x16
 * (16-bit PCM, converted in the kernel as s / 32768, which is exact) is non-NULL.  y is fp32 (B, Lcap): y[b, :L_b] is
 * exactly what air_ir_convolve writes for that utterance alone with L = L_b - the convolution truncated at L_b and, with
 * normalize, max|x| and max|y| taken over [0, L_b) only - and y[b, L_b:] is written as 0.  ir_idx[b] < 0 copies
 * x[b, :L_b] (converted, for x16) and zeroes the tail.  No input sample at index >= L_b is read.  The lengths are device
 * data and nothing synchronises with the host, so the call can be captured in a graph.  The same kernels as the dense
 * entry point (templated on the sample type, the row length taking the place of L at staging and at the store), the
 * same route selection and the same workspace (air_ir_convolve_ws_bytes[_ex]): ONE convolution launch for the whole
 * batch, its grid sized by Lcap, whose workgroups wholly behind L_b only write zeros and return; the rescale launch
 * (normalize) and, on the FFT route, the two table launches as in the dense call.  A NULL lengths_dev, both or neither
 * of x / x16, x == y or a non-positive size: AIR_EINVAL, ahead of any HIP call; normalize with a workspace below
 * air_ir_convolve_ws_bytes(B): AIR_EWORKSPACE. */
int air_ir_convolve_ragged(const float* x, const int16_t* x16, int B, int Lcap, const int* lengths_dev,
                           const float* irs, int n_ir, int H, const int* ir_idx, int normalize,
                           float* y, void* ws, size_t ws_bytes, air_stream_t stream);
/* A BANK of responses of different lengths, each up to 65 536 taps (room responses: tenths of a second to seconds), on a
 * dense or ragged batch.  Rows, lengths (a NULL pointer: the dense batch, L_b = Lcap), the x / x16 choice, ir_idx[b] < 0,
 * the zero tail y[b, L_b:], normalize and the two peaks per row at the head of the workspace are exactly as in
 * air_ir_convolve_ragged.  irs is (n_ir, Hmax) fp32; ir_taps_dev[i] is DEVICE data, clamped by the kernels into
 * [1, Hmax]: the leading taps_i columns of row i are the response, columns at or behind it are never read (they may hold
 * anything).  y[b, :L_b] = (x_b * irs[i, :taps_i])[:L_b], i = ir_idx[b]; each row pays for its own response only:
 *   taps_i <= 1025: the overlap-save form of air_ir_convolve_ragged (two 3072-sample blocks per 4096-point transform) -
 *     the same device code, so the row carries, bit for bit, what that call gives with the bank's first 1025 columns
 *     zeroed behind taps_i;
 *   taps_i > 1025: uniformly partitioned overlap-save - 4096-point transforms, the response cut into partitions of 2048
 *     taps, the hop 2048 samples; every pair of input segments is transformed once into the workspace, an output pair
 *     accumulates (segment spectrum x partition spectrum) over the row's own ceil(taps_i / 2048) partitions in registers
 *     and takes one inverse transform.
 * Nothing depends on Lcap, B or the other rows: y[b, :L_b] carries the bits of the call on that utterance alone.
 * Lengths, indices and tap counts are device data and nothing synchronises with the host, so the call can be captured in
 * a graph and replayed after they are rewritten; the peaks are cleared by a kernel; the twiddle and partition-spectra
 * tables are rebuilt per call, so the bank may be rewritten in place between calls.  Launches: [clear peaks,] twiddles,
 * partition spectra (ceil(Hmax / 2048) x n_ir workgroups), segment spectra (only with Hmax > 1025), convolve [, rescale];
 * the grids are sized by Lcap and Hmax, workgroups of partitions a response does not have, of rows on the other form and
 * of blocks behind L_b return at once.  Workspace: air_ir_bank_ws_bytes (peaks + tables + with Hmax > 1025 the segment
 * spectra, B x 2 x ceil(Lcap / 4096) x 32 KB); 0 for arguments the call refuses.  Hmax > 65536, a NULL ir_taps_dev, irs
 * or y, both or neither of x / x16, x == y, a non-positive size (or B, n_ir above 65535): AIR_EINVAL, ahead of any HIP
 * call; a workspace below air_ir_bank_ws_bytes: AIR_EWORKSPACE. */
size_t air_ir_bank_ws_bytes(int B, int Lcap, int n_ir, int Hmax);
int air_ir_bank_convolve(const float* x, const int16_t* x16, int B, int Lcap, const int* lengths_dev_or_null,
                         const float* irs, int n_ir, int Hmax, const int* ir_taps_dev, const int* ir_idx,
                         int normalize, float* y, void* ws, size_t ws_bytes, air_stream_t stream);

/* G.711 transmission codec ahead of the IR convolution - the first half of channel_simulation/simulated_device_channel.py:
 * 47-54 (codec, then device), for the two sample-parallel entries of the reference's codec list, G.711 mu-law and A-law
 * (the adaptive-predictor and whole-file codecs of that list are not covered).  Rows as in air_ir_convolve_ragged:
 * exactly one of x (fp32) / x16 (16-bit PCM, s / 32768) is non-NULL, row b = x + b * Lcap holds L_b = clamp(lengths[b],
 * 1, Lcap) samples; a NULL lengths pointer means L_b = Lcap for every row (the dense batch).  law_idx[b] < 0 copies
 * x[b, :L_b] (converted, for x16); 0 is mu-law; 1 - and anything above, the index being caller data - A-law; a NULL
 * law_idx is mu-law for every row.  fir is a DEVICE array of ntaps coefficients, ntaps odd in [1, 127], c = (ntaps-1)/2.
 *   resample != 0, with M_b = ceil(L_b / 2):
 *     1. u[m] = sum_k fir[k] x[2 m + c - k], m in [0, M_b), x taken as 0 outside [0, L_b); fp32, k ascending;
 *     2. s = clamp(rint(u * 32768), -32768, 32767) (ties to even), code = G.711 encode(s), d = G.711 decode(code):
 *        the integer arithmetic of ITU-T G.711 as CPython's audioop states it (mu-law on the top 14 bits of s, A-law on
 *        the top 13), bit for bit on all 65 536 values of s;
 *     3. v[m] = d / 32768;
 *     4. y[n] = 2 sum_k fir[k] vup[n + c - k], n in [0, L_b), vup[2 m] = v[m], 0 at odd positions and outside
 *        [0, 2 M_b) - evaluated in polyphase form, the stuffed zeros are never multiplied;
 *   resample == 0: steps 2 and 3 on every input sample at its own rate (M_b = L_b, y[n] = v[n]); fir and ntaps are only
 *     checked;
 *   either way, normalize != 0 then rescales each coded row to its input peak over [0, L_b), as air_ir_convolve does.
 * y is fp32 (B, Lcap), y[b, L_b:] = 0; no input at index >= L_b is read.  codes_or_null, if given, receives the 8-bit
 * codes of step 2 - (B, (Lcap + 1) / 2) with resample, (B, Lcap) without - with the tail behind M_b and every
 * pass-through row written as 0.  Nothing depends on Lcap or on the other rows: y[b, :L_b] carries the bits of the call
 * on that utterance alone.  Lengths and law indices are device data and nothing synchronises with the host, so the call
 * can be captured in a graph.  ONE launch for the whole batch (grid sized by Lcap; a workgroup stages its 2048 outputs'
 * input span plus the halo of both filters in LDS, recomputes the 8 kHz samples of the halo, and writes zeros and returns
 * when it lies wholly behind L_b); with normalize, a small launch that clears the peaks in front of it (a kernel rather
 * than a memset, so that the captured call replays) and the rescale launch behind it.  Both or neither of x / x16, x == y, a NULL y, a
 * non-positive size, an even ntaps or one outside [1, 127], resample with a NULL fir: AIR_EINVAL, ahead of any HIP call;
 * normalize with a workspace below air_g711_ws_bytes(B): AIR_EWORKSPACE. */
size_t air_g711_ws_bytes(int B);
int air_g711_ragged(const float* x, const int16_t* x16, int B, int Lcap, const int* lengths_dev_or_null,
                    const float* fir, int ntaps, const int* law_idx, int resample, int normalize,
                    float* y, uint8_t* codes_or_null, void* ws, size_t ws_bytes, air_stream_t stream);

/* RawBoost (Tak et al., ICASSP 2022) - the raw-waveform augmentation of the ASVspoof 2021 LA / DF baselines - on a dense
 * or ragged batch.  Parity with the authors' script and its numpy stream is NOT claimed; this text is the specification.
 * Rows as in air_g711_ragged: exactly one of x (fp32) / x16 (16-bit PCM, s / 32768), row b holds L_b = clamp(lengths[b],
 * 1, Lcap) samples, a NULL lengths pointer is the dense batch; y is fp32 (B, Lcap), y[b, L_b:] = 0, nothing at or behind
 * L_b is read.  fs = 16000.
 *
 * The parameter table is DEVICE data, (B, 164) doubles, every entry a value a double holds exactly:
 *   [0] algorithm: 0 LnL, 1 ISD, 2 SSI, 3 LnL -> ISD -> SSI, 4 LnL -> ISD, 5 LnL -> SSI, 6 ISD -> SSI,
 *       7 N0(LnL(x) + ISD(x)); anything else copies the row (converted, for x16)
 *   [1] T = floor(beta / 100 * 2^32), the ISD threshold     [2] g_sd          [5] SNR in dB
 *   [3] isd_base, [4] ssi_base: the call's Philox counter bases (below)       [6] ISD key, [7] SSI key
 *   [8 + 26 s ..], s = 0 .. 5, filter slot s: [G in dB, nBands (0: slot unused, at most 8), (fc, bw, c) x 8];
 *       slots 0 .. 4 are b_0 .. b_4 of the LnL stage (an unused one adds nothing), slot 5 is the SSI filter.
 *
 * Notch cascade b = notch(slot) (air_rawboost_design; fp64 on the device, rounded to fp32 once).  Per band, c odd:
 *   f1 = fc - bw / 2 (1/1000 if <= 0), f2 = fc + bw / 2 (fs/2 - 1/1000 if >= fs/2), l = f1 / (fs/2), r = f2 / (fs/2),
 *   m = k - (c - 1) / 2, h[k] = (l sinc(l m) + sinc(m) - r sinc(r m)) (0.54 - 0.46 cos(2 pi k / (c - 1))), h /= sum(h)
 *   - scipy.signal.firwin(c, [f1, f2], window='hamming', fs=fs); b = the linear convolution of the bands' h (sum c -
 *   (nBands - 1) taps, at most 512), times 10^(G / 20) / max_k |H(k pi / 512)|, k = 0 .. 511.  A slot whose c is even or
 *   outside [1, 512], or whose cascade exceeds 512 taps, gets no taps (length 0).
 * Centred FIR: F(b, v)[n] = sum_k b[k] v[n + (len(b) + 1) / 2 - k], n in [0, L_b), v = 0 outside [0, L_b).
 * Peak rule: N0(y) = y / max|y| if max|y| > 1, else y (an fp32 division by the fp32 peak).
 *   LnL  y = sum_i F(b_i, p_{i+1}), p_1 = x, p_{j+1} = fl32(p_j x) (fp32, this order); y -= (float) mean(y); N0.
 *        One fmaf chain per output over all filters' taps (the order of the terms is not part of the specification).
 *   ISD  sample j is selected iff word 0 of the Philox4x32-10 block at counter isd_base + b Lcap + j, key [6], is < T;
 *        then y[j] = x[j] + (g x[j]) ((2 u1 - 1) (2 u2 - 1)), u_i = fl32(word i) 2^-32, each operation rounded to
 *        fp32; else y[j] = x[j]; N0.  (The authors take exactly int(L beta / 100) distinct positions.)
 *   SSI  n = the standard normals air_randn(seed = key [7], offset = ssi_base + b ceil(Lcap / 4)) would write, element j
 *        for sample j; q = F(b_5, n); y = fmaf(q, s, x), s = (float)(||x|| / (||q|| 10^(SNR / 20))) from fp64 norms;
 *        ||q|| = 0 gives y = x.  No peak rule behind it.
 * Row statistics (sum, max |.|, sum of squares) are per-tile partials in a fixed order, merged in fp64 over the row's
 * own tiles; no floating-point atomics.  The tiling (air_rawboost_tile() samples, by sample index) depends on the row
 * alone: a call repeats its bits, and row b carries the bits of the dense call on that utterance alone whose table row
 * has isd_base + b Lcap and ssi_base + b ceil(Lcap / 4) in [3] and [4].
 * Random streams: the host holds the two bases and advances them per call - ISD by B 2^20 (Lcap <= 2^20 is enforced, so
 * a call's counters [isd_base, isd_base + B Lcap) stay inside its reservation), SSI by B 2^18 quads; the two stages use
 * different keys, so no two streams of any two calls overlap; bases stay below 2^53.
 * Launches: design (6 B workgroups), LnL FIR, SSI FIR, centre, three pointwise passes - 7, back to back on the stream,
 * no host synchronisation, so the call can be captured.  air_rawboost_ws_bytes: taps + three (B, Lcap) fp32 buffers +
 * the partials; 0 for sizes the call refuses.  air_rawboost_design alone writes taps (6 B, 512) fp32 and lens (6 B)
 * int32, slot s of row b at index 6 b + s - the bits the full call uses.  air_rawboost_row_doubles() = 164.
 * Both or neither of x / x16, x == y, a NULL y or table, B outside [1, 65535], Lcap outside [1, 2^20]: AIR_EINVAL ahead
 * of any HIP call; a workspace below air_rawboost_ws_bytes: AIR_EWORKSPACE. */
int air_rawboost_tile(void);
int air_rawboost_row_doubles(void);
size_t air_rawboost_ws_bytes(int B, int Lcap);
int air_rawboost_design(const double* params, int B, float* taps, int* lens, air_stream_t stream);
int air_rawboost_ragged(const float* x, const int16_t* x16, int B, int Lcap, const int* lengths_dev_or_null,
                        const double* params, float* y, void* ws, size_t ws_bytes, air_stream_t stream);

/* --------------------------------------------------------------- conv1d --
 * nn.Conv1d (stride 1) as used by ecapa_tdnn.py:39,46,55,111,118,140,143, with the
 * conv -> ReLU -> BN ordering of ecapa_tdnn.py:67-69 supported by bias / ReLU epilogues.
 * x (B, Cin, T), w (Cout, Cin, K), y (B, Cout, T).  Supported: K=1; K=3 with
 * dilation 2..4 and pad = dilation; K=5 with pad 2.  x_bstride / y_bstride are batch
 * strides in floats (0 = contiguous) so channel groups of a wider tensor (the Res2
 * split, the (x1,x2,x3) concat) are addressed in place.
 */
typedef struct AirConv1d {
  int B, Cin, T, Cout, K, dil, pad;
  size_t x_bstride, y_bstride;
} AirConv1d;

size_t air_conv1d_ws_bytes(const AirConv1d* p);
/* y = relu?(conv1d(x, w) + bias[co] + bias_bc[b][co]); bias, bias_bc may be NULL. */
int air_conv1d_fwd(const AirConv1d* p, const float* x, const float* w, const float* bias,
                   const float* bias_bc, int relu, float* y, void* ws, size_t ws_bytes,
                   air_stream_t stream);
int air_conv1d_dgrad(const AirConv1d* p, const float* dy, const float* w, float* dx,
                     const float* accumulate, void* ws, size_t ws_bytes, air_stream_t stream);
int air_conv1d_wgrad(const AirConv1d* p, const float* x, const float* dy, float* dw, void* ws,
                     size_t ws_bytes, air_stream_t stream);

/* bf16-compute variants of the pointwise (K = 1) layers (BASELINE.json configs[2], "ECAPA-TDNN-512
 * bf16 train"): ecapa_tdnn.py:39,55,118,140,143.  Same tensors (fp32 in HBM), same epilogues;
 * both operands are rounded to bf16 (nearest even) as they are staged, products accumulate in
 * fp32 on v_mfma_f32_32x32x16_bf16 - the arithmetic of torch.autocast(bfloat16) for nn.Conv1d.
 * air_conv1d_bf16_supported(p, pass): pass 0 forward (Cout % 128 == 0, Cin % 32 == 0),
 * 1 dgrad (Cin % 128 == 0, Cout % 32 == 0), 2 wgrad (Cout % 128 == 0, Cin % 128 == 0); 1 = yes.
 * Other layers (K = 3 dilated, K = 5) stay on the fp32 entry points above. */
int air_conv1d_bf16_supported(const AirConv1d* p, int pass);
size_t air_conv1d_bf16_ws_bytes(const AirConv1d* p);
int air_conv1d_fwd_bf16(const AirConv1d* p, const float* x, const float* w, const float* bias,
                        const float* bias_bc, int relu, float* y, void* ws, size_t ws_bytes,
                        air_stream_t stream);
/* Same, and y is also written as bf16 (nearest even) into y_bf16[(b*Cout + c) * air_conv1d_bf16_tp(T) + t], the
 * operand layout of air_conv1d_wgrad_bf16_pre (from the GEMM's epilogue for the wide layers, by a conversion
 * pass otherwise); NULL = air_conv1d_fwd_bf16. */
int air_conv1d_fwd_bf16_ex(const AirConv1d* p, const float* x, const float* w, const unsigned short* w_packed,
                           const float* bias, const float* bias_bc, int relu, float* y, unsigned short* y_bf16,
                           void* ws, size_t ws_bytes, air_stream_t stream);
/* K = 3 layers: the kernels read the weights as bf16 [tap][m][k] (dgrad: transposed, taps flipped).  The
 * _bf16 entry points pack them on every call; air_conv1d_tap_pack_bf16 packs n_layers equally shaped layers
 * (weights w_stride floats apart, e.g. the seven Res2 branch convs of a Bottle2neck inside the parameter arena)
 * in ONE launch, layer i at out + i * air_conv1d_tap_pack_elems(Cout, Cin); pass that block as w_packed (w may
 * then be NULL).  w_packed must be NULL for K = 1 layers. */
size_t air_conv1d_tap_pack_elems(int Cout, int Cin);
int air_conv1d_tap_pack_bf16(const float* w, size_t w_stride, int n_layers, int Cout, int Cin, int transpose,
                             unsigned short* out, air_stream_t stream);
int air_conv1d_dgrad_bf16(const AirConv1d* p, const float* dy, const float* w, float* dx,
                          const float* accumulate, void* ws, size_t ws_bytes, air_stream_t stream);
/* Forward (dgrad = 0: y = W . x) or data gradient (dgrad = 1: dx = W^T . dy + accumulate) of a K = 1 layer whose INPUT
 * operand the caller already holds as a bf16 copy in the weight-gradient layout [b][channel][Tp] (xb, batch stride
 * xb_bstride in elements, 0 = dense): the 256 x 256 GEMM reads it K-major (ds_read_b64_tr_b16), so neither a
 * conversion nor a transposed copy is made - the SAME copy serves this layer's forward, its data gradient's
 * counterpart and the weight gradients around it.  Needs Cout % 256 == 0 (forward) / Cin % 256 == 0 (dgrad), the K
 * dimension a multiple of 64 and Tp % 256 == 0; AIR_EUNSUPPORTED otherwise.  accumulate / accumulate2 (either may be
 * NULL) with their batch strides in floats (0 = the output's), as in air_conv1d_dgrad_bf16_ex; y_bf16 as in
 * air_conv1d_fwd_bf16_ex. */
int air_conv1d_pointwise_bf16_kmajor(const AirConv1d* p, const unsigned short* xb, size_t xb_bstride, const float* w,
                                     int dgrad, const float* bias, const float* bias_bc, int relu,
                                     const float* accumulate, size_t acc_bstride, const float* accumulate2,
                                     size_t acc2_bstride, float* y, unsigned short* y_bf16, void* ws, size_t ws_bytes,
                                     air_stream_t stream);
/* Same with up to two accumulate operands, each with its own batch stride in floats (0 = dx's): dx = dgrad +
 * accumulate + accumulate2.  ECAPA's block input gradient = dgrad(conv1) + d(block output) [the residual,
 * ecapa_tdnn.py:93] + the (B, 1536, T) concat gradient's slice for the previous block [:170] in one epilogue.
 * AIR_EUNSUPPORTED for the K = 3 and the wide-layer paths when a second operand or a foreign stride is given. */
int air_conv1d_dgrad_bf16_ex(const AirConv1d* p, const float* dy, const float* w, const unsigned short* w_packed,
                             float* dx, const float* accumulate, size_t acc_bstride, const float* accumulate2,
                             size_t acc2_bstride, void* ws, size_t ws_bytes, air_stream_t stream);
int air_conv1d_wgrad_bf16(const AirConv1d* p, const float* x, const float* dy, float* dw, void* ws,
                          size_t ws_bytes, air_stream_t stream);
/* The weight-gradient GEMM runs on bf16 copies of its operands, [b][channel][Tp] with
 * Tp = air_conv1d_bf16_tp(T) frames per row and zeros for t >= T; air_conv1d_wgrad_bf16 makes them in its
 * workspace, one HBM pass per operand.  A caller that already holds a copy - written by the tensor's producer
 * (air_bn_bwd_ex2's dx_bf16) or converted once with air_conv1d_cvt_bf16 for several layers (ECAPA's (B, 1536, T)
 * concat feeds layer4 and, as channel slices, two Bottle2neck conv1 layers: ecapa_tdnn.py:118,39) - passes it to
 * air_conv1d_wgrad_bf16_pre: x_bf16 / dy_bf16 with their batch strides in ELEMENTS (0 = dense; a channel slice
 * of a wider copy keeps the wide stride), NULL = convert the fp32 tensor as before.  Same rounding (nearest
 * even) everywhere, so results are bit-identical to air_conv1d_wgrad_bf16. */
int air_conv1d_bf16_tp(int T);
int air_conv1d_cvt_bf16(const float* x, size_t x_bstride, int B, int C, int T, unsigned short* out,
                        air_stream_t stream);
int air_conv1d_wgrad_bf16_pre(const AirConv1d* p, const float* x, const float* dy, const unsigned short* x_bf16,
                              size_t x_bf16_bstride, const unsigned short* dy_bf16, size_t dy_bf16_bstride,
                              float* dw, void* ws, size_t ws_bytes, air_stream_t stream);

/* ------------------------------------------------------- batchnorm/relu --
 * nn.BatchNorm2d/1d (+ F.relu) as used at resnet.py:55-67,132,142 and
 * ecapa_tdnn.py.  x is (B, C, S) with S = H*W (or T).
 */
/* Batch statistics -> mean/invstd, fused scale/shift for the apply, running
 * stat update (momentum 0.1, unbiased var) when running_* non-NULL.
 * stats_in: NULL - the kernel reduces x itself (shifted sums, fp64 two-stage, fixed order) - or the statistics
 * records air_conv2d_fwd wrote for this very tensor (its header carries the group and channel counts, which must
 * match C; x is then not read): a wave per channel merges them in fp64 in a fixed order (Chan's formula on
 * (n, mean, M2)). */
size_t air_bn_ws_bytes(int B, int C, int S);
int air_bn_stats(const float* x, int B, int C, int S, const double* stats_in,
                 const float* gamma, const float* beta, float eps, float momentum,
                 float* running_mean, float* running_var,
                 float* mean, float* invstd, float* scale, float* shift,
                 void* ws, size_t ws_bytes, air_stream_t stream);
/* Eval-mode scale/shift from running stats. */
int air_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean,
                       const float* running_var, float eps, int C, float* scale, float* shift,
                       air_stream_t stream);
/* y = x*scale[c] + shift[c], optional ReLU. */
int air_bn_apply(const float* x, int B, int C, int S, const float* scale, const float* shift,
                 int relu, float* y, air_stream_t stream);
/* Same, and rowmean[b*C + c] (B*C floats, may be NULL) receives the mean over s of the OUTPUT plane: the SE
 * squeeze (ecapa_tdnn.py:19) of the tensor being written, without a pass that re-reads it.  rowmean needs
 * 32 <= S <= 1024 (one workgroup per plane); AIR_EUNSUPPORTED otherwise.  y_bf16 (may be NULL): y also as bf16 at
 * y_bf16[(b*C + c) * y_bf16_tp + s], the operand layout of air_conv1d_wgrad_bf16_pre. */
int air_bn_apply_ex(const float* x, int B, int C, int S, const float* scale, const float* shift,
                    int relu, float* y, float* rowmean, unsigned short* y_bf16, int y_bf16_tp, air_stream_t stream);
/* Backward of y = relu?(bn(x)) in training mode.  dy: grad wrt y.  relu bit 0: a ReLU
 * follows the BN (resnet.py:64); bit 1: the BN input is itself a ReLU output
 * (conv -> ReLU -> BN, ecapa_tdnn.py:67-69), so dx is masked where x == 0 and is the
 * gradient w.r.t. the pre-ReLU conv output.
 * dx_accum: if non-zero dx += result (gradient joining a residual branch).
 * dgamma/dbeta: (C,) written. */
int air_bn_bwd(const float* x, const float* dy, int B, int C, int S,
               const float* mean, const float* invstd, const float* gamma, const float* beta,
               int relu, float* dx, int dx_accum, float* dgamma, float* dbeta,
               void* ws, size_t ws_bytes, air_stream_t stream);
/* Same with three fusions for the conv -> ReLU -> BN layers of ecapa_tdnn.py:
 *  - dy may be a channel-slice view (dy_bstride = batch stride in floats, 0 = dense) and a second gradient dy2
 *    (same shape, own batch stride, may be NULL) is added to it on the fly: the Res2 chain's
 *    "d(sp_i) = d(cat slice) + d(next branch input)" join (ecapa_tdnn.py:78-83) without a pass that forms the sum;
 *  - dy_rowbias (B*C) or NULL: the incoming gradient is dy + rowbias_scale * dy_rowbias[b][c] - the SE
 *    squeeze's mean-over-time gradient (ecapa_tdnn.py:19: d mean / d x = 1/T) without a pass that adds it;
 *  - dbias (C) or NULL (needs relu bit 1): gradient of the conv bias, sum_{b,s} dx, obtained in closed
 *    form from three extra sums of the statistics pass - no pass over dx. */
int air_bn_bwd_ex(const float* x, const float* dy, size_t dy_bstride, const float* dy2, size_t dy2_bstride,
                  const float* dy_rowbias, float rowbias_scale, int B, int C, int S, const float* mean,
                  const float* invstd, const float* gamma, const float* beta, int relu, float* dx, int dx_accum,
                  float* dgamma, float* dbeta, float* dbias, void* ws, size_t ws_bytes, air_stream_t stream);
/* Same, and dx is also written as bf16 (nearest even) into dx_bf16[(b*C + c) * dx_bf16_tp + s] - the operand
 * layout of air_conv1d_wgrad_bf16_pre (dx_bf16_tp = air_conv1d_bf16_tp(S); the caller keeps the frames
 * s >= S zero).  dx_bf16 NULL = air_bn_bwd_ex. */
int air_bn_bwd_ex2(const float* x, const float* dy, size_t dy_bstride, const float* dy2, size_t dy2_bstride,
                   const float* dy_rowbias, float rowbias_scale, int B, int C, int S, const float* mean,
                   const float* invstd, const float* gamma, const float* beta, int relu, float* dx, int dx_accum,
                   float* dgamma, float* dbeta, float* dbias, unsigned short* dx_bf16, int dx_bf16_tp, void* ws,
                   size_t ws_bytes, air_stream_t stream);
/* air_bn_bwd_ex2 with the two per-channel sums taken by the convolution that produced dy (air_conv2d_dgrad_bn,
 * `sums`): the first pass over (x, dy) is skipped, a workgroup per channel merges the records in fp64.  sums_in NULL =
 * air_bn_bwd_ex2.  Only for plain relu(batchnorm(x)) with one dense gradient (dy2, dy_rowbias, dbias NULL, relu = 1). */
int air_bn_bwd_ex3(const float* x, const float* dy, size_t dy_bstride, const float* dy2, size_t dy2_bstride,
                   const float* dy_rowbias, float rowbias_scale, int B, int C, int S, const float* mean,
                   const float* invstd, const float* gamma, const float* beta, int relu, float* dx, int dx_accum,
                   float* dgamma, float* dbeta, float* dbias, unsigned short* dx_bf16, int dx_bf16_tp,
                   const void* sums_in, void* ws, size_t ws_bytes, air_stream_t stream);

/* ------------------------------------------------------------- pooling ---
 * SelfAttention.forward (resnet.py:23-46) on x (B, C, T) (the squeezed conv5
 * output, i.e. BEFORE the permute at resnet.py:185): w_t = <x[:, :, t], a>,
 * alpha = softmax_T(tanh(w)), weighted = x*alpha, out = [sum_T weighted ,
 * unbiased std_T(weighted + noise)] -> (B, 2C).
 * noise: NULL (none) or (B, T, C) already scaled by 1e-5 (reference layout).
 */
int air_selfatt_pool_fwd(const float* x, int B, int C, int T, const float* att_w,
                         const float* noise, float* out, float* alpha_save, air_stream_t stream);
int air_selfatt_pool_bwd(const float* x, int B, int C, int T, const float* att_w,
                         const float* noise, const float* alpha, const float* out,
                         const float* dout, float* dx, float* datt_partial /*(B,C)*/,
                         air_stream_t stream);

/* out[n] = sum_m x[m][n]: folds the per-utterance datt partials over the batch. */
int air_sum_rows(const float* x, int M, int N, float* out, air_stream_t stream);
/* scale * N(0,1) from a Philox4x32-10 counter stream (seed, offset): the on-device
 * replacement for the host-side ``1e-5*torch.randn`` of resnet.py:38. */
int air_randn(float* out, size_t n, uint64_t seed, uint64_t offset, float scale,
              air_stream_t stream);
/* The same draw with the stream offset held in DEVICE memory: reads *counter as the offset and advances it by
 * ceil(n / 4) behind the draw (a second, 1-thread launch on the same stream).  resnet.py:38 draws fresh noise on
 * every call; inside a captured hipGraph a host-side offset would be frozen into the graph, a device-side one is
 * not - eager launches and graph replays walk the same (seed, offset) sequence.  counter: 8-byte aligned. */
int air_randn_ctr(float* out, size_t n, uint64_t seed, uint64_t* counter, float scale, air_stream_t stream);

/* --------------------------------------------------------------- linear ---
 * nn.Linear (resnet.py:143-144,187-189; ecapa_tdnn.py:148-149): y = x W^T + b.
 * x (M,K), w (N,K), y (M,N).
 */
int air_linear_fwd(const float* x, const float* w, const float* b, int M, int K, int N, float* y,
                   air_stream_t stream);
int air_linear_relu_fwd(const float* x, const float* w, const float* b, int M, int K, int N,
                        float* y, air_stream_t stream); /* y = max(0, x W^T + b) */
int air_linear_bwd(const float* x, const float* w, const float* dy, int M, int K, int N,
                   float* dx, float* dw, float* db, air_stream_t stream);

/* ------------------------------------------------------ ECAPA small ops ---
 * (B, C, T) fp32, time contiguous; *_bstride = batch stride in floats (0 = contiguous).
 */
/* out = a (+ b): copies / joins channel groups that are views of wider tensors
 * (torch.split / torch.cat / "sp + spx[i]" of ecapa_tdnn.py:71-83). */
int air_add_strided(float* out, size_t out_bstride, const float* a, size_t a_bstride,
                    const float* b, size_t b_bstride, int B, int C, int S, air_stream_t stream);
/* Res2 chain step (ecapa_tdnn.py:78-83): v = x*scale[c] + shift[c]; y1 = v (a channel slice of the
 * concat tensor, batch stride y1_bstride); optional y2 = v + add (dense; add is a channel slice with
 * batch stride add_bstride): the next branch's input "sp + spx[i+1]".  add and y2 both NULL or both set. */
int air_res2_bn_apply(const float* x, int B, int C, int S, const float* scale, const float* shift, float* y1,
                      size_t y1_bstride, const float* add, size_t add_bstride, float* y2, air_stream_t stream);
/* Both with a bf16 copy of the result (out / y1) in the weight-gradient operand layout of
 * air_conv1d_wgrad_bf16_pre: element (b, c, s) at bf16[b * bstride + c * tp + s], bstride in elements (0 = C * tp),
 * tp = air_conv1d_bf16_tp(S); the seven branch outputs and the pass-through group of a Bottle2neck together fill
 * the bf16 copy of its concat (conv3's X operand).  NULL = the plain entry points. */
int air_add_strided_ex(float* out, size_t out_bstride, const float* a, size_t a_bstride, const float* b,
                       size_t b_bstride, int B, int C, int S, unsigned short* out_bf16, size_t out_bf16_bstride,
                       int out_bf16_tp, air_stream_t stream);
int air_res2_bn_apply_ex(const float* x, int B, int C, int S, const float* scale, const float* shift, float* y1,
                         size_t y1_bstride, const float* add, size_t add_bstride, float* y2, unsigned short* y1_bf16,
                         size_t y1_bf16_bstride, int y1_bf16_tp, air_stream_t stream);
/* out[c] = sum_{b,s} x[b][c][s]: conv bias gradients (fp64 partials, fixed order). */
size_t air_channel_sum_ws_bytes(int B, int C);
int air_channel_sum(const float* x, int B, int C, int S, size_t bstride, float* out, void* ws,
                    size_t ws_bytes, air_stream_t stream);
/* mean_T and sqrt(clamp(var_T unbiased, clamp_min)) per (b,c) row: SE squeeze
 * (ecapa_tdnn.py:19) and the context statistics (:178).  std may be NULL. */
int air_row_stats(const float* x, int B, int C, int T, float* mean, float* std_or_null,
                  float clamp_min, air_stream_t stream);
/* dx (+)= dmean/T + dstd * (x - mean) / ((T-1) std).  relu_mask != 0: x is a ReLU output and the result
 * is zeroed where x == 0 (the stand-alone ReLU after layer4, ecapa_tdnn.py:173, folded in);
 * rowsum (B*C) or NULL: sum over time of each result row (summed over b it is the conv bias gradient). */
int air_row_stats_bwd(const float* x, int B, int C, int T, const float* mean, const float* std_,
                      const float* dmean, const float* dstd, float clamp_min, float* dx,
                      int accumulate, int relu_mask, float* rowsum_or_null, air_stream_t stream);
/* Same, and the result is also written as bf16 into dx_bf16[(b*C + c) * dx_bf16_tp + t] (operand layout of
 * air_conv1d_wgrad_bf16_pre; NULL = air_row_stats_bwd). */
int air_row_stats_bwd_ex(const float* x, int B, int C, int T, const float* mean, const float* std_,
                         const float* dmean, const float* dstd, float clamp_min, float* dx,
                         int accumulate, int relu_mask, float* rowsum_or_null, unsigned short* dx_bf16,
                         int dx_bf16_tp, air_stream_t stream);
/* dx *= (y > 0): backward of the stand-alone ReLU after layer4 (ecapa_tdnn.py:173). */
int air_relu_mask(float* dx, const float* y, size_t n, air_stream_t stream);
/* out[b][c] = sum_t x[b][c][t]: gradient of a per-utterance bias. */
int air_row_sum(const float* x, int B, int C, int T, float* out, air_stream_t stream);
/* SEModule gate + block residual (ecapa_tdnn.py:27-29,:93): out = x*sigmoid(z[b][c]) + res. */
int air_se_scale_fwd(const float* x, const float* z, const float* res, size_t res_bstride, int B,
                     int C, int T, float* out, size_t out_bstride, air_stream_t stream);
/* Same, with a bf16 copy of out at out_bf16[b * bstride + c * tp + t] (bstride in elements, 0 = C * tp): a block's
 * output is a channel slice of the (B, 1536, T) concat, and this fills the matching slice of the concat's bf16 copy. */
int air_se_scale_fwd_ex(const float* x, const float* z, const float* res, size_t res_bstride, int B,
                        int C, int T, float* out, size_t out_bstride, unsigned short* out_bf16,
                        size_t out_bf16_bstride, int out_bf16_tp, air_stream_t stream);
int air_se_scale_bwd(const float* x, const float* z, const float* dout, size_t dout_bstride, int B,
                     int C, int T, float* dx, float* dz, air_stream_t stream);
/* Attentive statistics pooling (ecapa_tdnn.py:143-185): softmax over T of the attention
 * logits (overwritten with the weights w), mu = sum x w, sg = sqrt(clamp(sum x^2 w - mu^2,
 * 1e-4)); out (B, 2C) = [mu | sg].  bwd overwrites w with d(logits). */
int air_asp_fwd(const float* x, float* logits_to_w, int B, int C, int T, float* out,
                air_stream_t stream);
/* rowsum_or_null (B*C): sum over time of each d(logits) row (summed over b: attention.3's bias gradient). */
int air_asp_bwd(const float* x, float* w_to_dlogits, int B, int C, int T, const float* out,
                const float* dout, float* dx, int accumulate, float* rowsum_or_null, air_stream_t stream);
/* Same, and d(logits) is also written as bf16 into dlogits_bf16[(b*C + c) * dlogits_bf16_tp + t] (NULL = air_asp_bwd). */
int air_asp_bwd_ex(const float* x, float* w_to_dlogits, int B, int C, int T, const float* out,
                   const float* dout, float* dx, int accumulate, float* rowsum_or_null,
                   unsigned short* dlogits_bf16, int dlogits_bf16_tp, air_stream_t stream);

/* ------------------------------------------- bf16-resident activations ---
 * BASELINE.json configs[2] ("ECAPA-TDNN-512 bf16 train"), round 3: every (B, C, T) activation between the layers
 * of ecapa_tdnn.py:64-95,152-187 lives in HBM as bf16 rows - element (b, c, t) at p[b * bs + c * Tp + t] with
 * Tp = air_h_tp(T) frames per row (a multiple of 256) and the frames T .. Tp - 1 ZERO; bs = batch stride in
 * ELEMENTS (0 = C * Tp), so channel slices of wider tensors (the Res2 split, the concats) are addressed in place.
 * Every entry point reads bf16, computes in fp32 and rounds each stored value once (nearest even) - the tensors
 * torch.autocast(bfloat16) would hold in bf16; what is rounded where is stated by oracle/ecapa.py
 * (bf16 = "resident").  Statistics, per-channel / per-row vectors, parameters and their gradients stay fp32.
 * Every writer keeps the padding zero; the GEMMs read the rows as operands without masks. */
int air_h_tp(int T);
/* K = 1 Conv1d (ecapa_tdnn.py:39,55,118,140,143) on bf16 rows, 256 x 256 bf16-MFMA GEMM reading x K-major:
 * dgrad = 0: y = relu?(W x + bias[co] + bias_bc[b][co]) (+ acc + acc2); dgrad = 1: dx = W^T dy + acc + acc2
 * (w is always the layer's (Cout, Cin, 1) fp32 weight; packed to bf16 into ws).  acc / acc2: bf16 rows of the
 * OUTPUT's channel count with their own batch strides, or NULL.  K (= Cin, or Cout for dgrad) % 64 == 0. */
size_t air_h_conv1d_ws_bytes(int Cout, int Cin);
int air_h_conv1d_pointwise(int B, int Cin, int Cout, int T, int Tp, const unsigned short* x, size_t x_bs, const float* w,
                           int dgrad, const float* bias, const float* bias_bc, int relu, const unsigned short* acc,
                           size_t acc_bs, const unsigned short* acc2, size_t acc2_bs, unsigned short* y, size_t y_bs,
                           void* ws, size_t ws_bytes, air_stream_t stream);
/* Same, and the epilogue that stores y also leaves the BatchNorm statistics of the STORED tensor (the conv -> ReLU ->
 * BatchNorm1d pairs of ecapa_tdnn.py:67-69,87-89,159-161,148-150) as {sum, sum of squares} per (channel, 64-frame
 * segment) in `stats` (air_h_conv1d_pointwise_stats_bytes(B, Cout, Tp) bytes, 8-byte aligned; NULL = the plain call);
 * air_h_bn_stats_ex takes it as stats_in.  Forward launches only (dgrad = 0). */
size_t air_h_conv1d_pointwise_stats_bytes(int B, int Cout, int Tp);
int air_h_conv1d_pointwise_ex(int B, int Cin, int Cout, int T, int Tp, const unsigned short* x, size_t x_bs,
                              const float* w, int dgrad, const float* bias, const float* bias_bc, int relu,
                              const unsigned short* acc, size_t acc_bs, const unsigned short* acc2, size_t acc2_bs,
                              unsigned short* y, size_t y_bs, void* stats, void* ws, size_t ws_bytes,
                              air_stream_t stream);
/* dw[co][ci] = sum_{b,t} dy x (fp32 out, split-K in fixed order); ws >= air_conv1d_bf16_ws_bytes of the layer. */
int air_h_conv1d_wgrad(int B, int Cin, int Cout, int T, int Tp, const unsigned short* x, size_t x_bs,
                       const unsigned short* dy, size_t dy_bs, float* dw, void* ws, size_t ws_bytes, air_stream_t stream);
/* Dilated K = 3 conv of a Res2 branch (ecapa_tdnn.py:46), forward (relu?(W * x + bias)) or data gradient
 * (dgrad = 1: w_packed from air_conv1d_tap_pack_bf16(transpose = 1)). */
int air_h_conv1d_tap(int B, int Cin, int Cout, int T, int Tp, int dil, const unsigned short* x, size_t x_bs,
                     const unsigned short* w_packed, int dgrad, const float* bias, int relu, unsigned short* y, size_t y_bs,
                     air_stream_t stream);
/* Same, and the epilogue that stores y also leaves the BatchNorm statistics of the STORED tensor (ecapa_tdnn.py:47-48,
 * 79-81: conv -> ReLU -> BatchNorm1d of a Res2 branch) as {sum, sum of squares} per (channel, 32-frame segment) in
 * `stats` (air_h_conv1d_tap_stats_bytes(B, Cout, Tp) bytes, 8-byte aligned; NULL = air_h_conv1d_tap).  Hand it to
 * air_h_bn_stats_ex as stats_in and the BatchNorm makes no pass over y (round 4: 21 passes per ECAPA step). */
size_t air_h_conv1d_tap_stats_bytes(int B, int Cout, int Tp);
int air_h_conv1d_tap_ex(int B, int Cin, int Cout, int T, int Tp, int dil, const unsigned short* x, size_t x_bs,
                        const unsigned short* w_packed, int dgrad, const float* bias, int relu, unsigned short* y,
                        size_t y_bs, void* stats, air_stream_t stream);
/* Same, for the DATA-GRADIENT launches of the Res2 chain (ecapa_tdnn.py:79-85 backward): y = d(input of branch i) is
 * the second half of the gradient that enters the BatchNorm of branch i - 1 (the first half, bn_dy, is that branch's
 * slice of the concat gradient; bn_x is the BatchNorm's input, the branch's ReLU output).  The epilogue also leaves
 * the five sums of that BatchNorm's backward pass - sum g, sum g xhat, and over bn_x > 0: sum g, the count, sum xhat
 * (g = bn_dy + y as stored, xhat = (bn_x - mean) invstd) - per (channel, 32-frame segment) in bn_sums
 * (air_h_conv1d_tap_bwd_sums_bytes(B, C, Tp) bytes, 16-byte aligned; bn_x / bn_dy 16-byte aligned rows).  Hand it to
 * air_h_bn_bwd_ex as sums_in: the BatchNorm backward then makes no first pass over (bn_x, bn_dy, y).  bn_sums NULL =
 * air_h_conv1d_tap_ex. */
size_t air_h_conv1d_tap_bwd_sums_bytes(int B, int C, int Tp);
int air_h_conv1d_tap_ex2(int B, int Cin, int Cout, int T, int Tp, int dil, const unsigned short* x, size_t x_bs,
                         const unsigned short* w_packed, int dgrad, const float* bias, int relu, unsigned short* y,
                         size_t y_bs, void* stats, const unsigned short* bn_x, size_t bn_x_bs,
                         const unsigned short* bn_dy, size_t bn_dy_bs, const float* bn_mean, const float* bn_invstd,
                         void* bn_sums, air_stream_t stream);
/* Round 6: the Res2 chain's elementwise passes folded into the staging of the conv that consumes them
 * (ecapa_tdnn.py:78-83: `sp = sp + spx[i]; sp = convs[i](sp); sp = bns[i](relu(sp))` - the BatchNorm of branch i - 1
 * needs batch statistics, so it cannot go into the launch that produces r_{i-1}; it goes into the NEXT launch's
 * operand read instead).  Same arithmetic and the same rounding points as air_h_res2_bn_apply / air_h_bn_bwd followed
 * by air_h_conv1d_tap_ex2: every stored tensor is bit-identical (tests/test_ecapa_bf16_gpu.py).  64 -> 64 channels only
 * (air_h_conv1d_tap_pro_ok); pro NULL or kind 0 = air_h_conv1d_tap_ex2.
 *   kind 1 (forward, dgrad = 0): x = r_{i-1} (raw ReLU output of the previous branch).  y1 = bf16(x * pa[c] + pb[c])
 *     -> side1 (its slice of the concat); operand t = bf16(y1 + g0) (g0 = o1's slice i) -> side0 (kept for the weight
 *     gradient).  pa / pb = the BatchNorm's scale / shift.
 *   kind 2 (data gradient, dgrad = 1): x = r_i (the BatchNorm input of THIS branch), g = g0 (+ g1) the gradient of its
 *     output; operand dc = bf16(pc pb (g - pd / N - xhat pe / N)), xhat = (x - pa) pb, zero where x <= 0 -> side0 (the
 *     weight gradient's dy).  pa / pb / pc / pd / pe = mean / invstd / gamma / dbeta / dgamma (air_h_bn_bwd_ex with
 *     dx = NULL leaves dgamma / dbeta / dbias without the apply pass).
 * side0 / side1 must not alias x, g0 or g1 (those are read with a halo of `dil` frames by neighbouring workgroups). */
typedef struct AirTapPrologue {
  int kind;
  const unsigned short* g0; size_t g0_bs;
  const unsigned short* g1; size_t g1_bs;
  const float* pa; const float* pb; const float* pc; const float* pd; const float* pe;
  unsigned short* side0; size_t side0_bs;
  unsigned short* side1; size_t side1_bs;
} AirTapPrologue;
int air_h_conv1d_tap_pro_ok(int Cin, int Cout);
int air_h_conv1d_tap_pro(int B, int Cin, int Cout, int T, int Tp, int dil, const unsigned short* x, size_t x_bs,
                         const unsigned short* w_packed, int dgrad, const float* bias, int relu, unsigned short* y,
                         size_t y_bs, void* stats, const unsigned short* bn_x, size_t bn_x_bs,
                         const unsigned short* bn_dy, size_t bn_dy_bs, const float* bn_mean, const float* bn_invstd,
                         void* bn_sums, const AirTapPrologue* pro, air_stream_t stream);
/* Weight gradients of the n_branches dilated K = 3 convs of one Res2 block (ecapa_tdnn.py:46, W -> W channels,
 * padding = dilation) in ONE launch: dw[i] (W, W, 3) fp32 = sum_{b,t} dy[i][b][co][t] x[i][b][ci][t + (k - 1) dil],
 * bf16 MFMA over the resident operands (products exact, fp32 sums, fixed-order split over the utterances) - the
 * fp32 contraction of the widened operands without the widened copies.  x / dy / dw: HOST arrays of n_branches
 * device pointers, x_bs / dy_bs their batch strides in elements (NULL or 0 = W * Tp).  W % 64 == 0, dil in 2..4,
 * n_branches <= 16, Tp % 64 == 0; ws >= air_h_conv1d_tap_wgrad_ws_bytes(). */
size_t air_h_conv1d_tap_wgrad_ws_bytes(int n_branches, int B, int W);
int air_h_conv1d_tap_wgrad(int n_branches, int B, int W, int T, int Tp, int dil, const unsigned short* const* x,
                           const size_t* x_bs, const unsigned short* const* dy, const size_t* dy_bs, float* const* dw,
                           void* ws, size_t ws_bytes, air_stream_t stream);
/* BatchNorm1d, training mode: statistics of the bf16 tensor (fp64 two-stage sums, running-stat update) ... */
size_t air_h_bn_ws_bytes(int B, int C);
int air_h_bn_stats(const unsigned short* x, size_t x_bs, int B, int C, int T, int Tp, const float* gamma,
                   const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                   float* mean, float* invstd, float* scale, float* shift, void* ws, size_t ws_bytes,
                   air_stream_t stream);
/* stats_in / stats_bytes: the records air_h_conv1d_tap_ex wrote for x (merged in fp64, a workgroup per channel; x is
 * not read), or NULL / 0 = air_h_bn_stats. */
int air_h_bn_stats_ex(const unsigned short* x, size_t x_bs, int B, int C, int T, int Tp, const void* stats_in,
                      size_t stats_bytes, const float* gamma, const float* beta, float eps, float momentum,
                      float* running_mean, float* running_var, float* mean, float* invstd, float* scale, float* shift,
                      void* ws, size_t ws_bytes, air_stream_t stream);
/* ... y = bf16(x * scale[c] + shift[c]); rowmean (B*C, may be NULL) = mean over t of the STORED y (the SE squeeze) */
int air_h_bn_apply(const unsigned short* x, size_t x_bs, int B, int C, int T, int Tp, const float* scale,
                   const float* shift, unsigned short* y, size_t y_bs, float* rowmean, air_stream_t stream);
/* ... and its backward for conv -> ReLU -> BN (x = the BN input, a ReLU output; relu_in masks dx where x == 0):
 * incoming gradient dy + dy2 + rowbias_scale * dy_rowbias[b][c] as in air_bn_bwd_ex; dx bf16 (may alias dy);
 * dgamma / dbeta / dbias (C) fp32. */
int air_h_bn_bwd(const unsigned short* x, size_t x_bs, const unsigned short* dy, size_t dy_bs, const unsigned short* dy2,
                 size_t dy2_bs, const float* dy_rowbias, float rowbias_scale, int B, int C, int T, int Tp,
                 const float* mean, const float* invstd, const float* gamma, int relu_in, unsigned short* dx,
                 size_t dx_bs, float* dgamma, float* dbeta, float* dbias, void* ws, size_t ws_bytes,
                 air_stream_t stream);
/* (round 6) dx NULL: the sums / dgamma / dbeta / dbias only - the apply pass is the prologue of air_h_conv1d_tap_pro. */
/* sums_in / sums_bytes: the records air_h_conv1d_tap_ex2 wrote for this BatchNorm (merged in fp64, a workgroup per
 * channel; the first pass over x / dy / dy2 is skipped), or NULL / 0 = air_h_bn_bwd.  Needs relu_in = 1, no row bias. */
int air_h_bn_bwd_ex(const unsigned short* x, size_t x_bs, const unsigned short* dy, size_t dy_bs, const unsigned short* dy2,
                    size_t dy2_bs, const float* dy_rowbias, float rowbias_scale, int B, int C, int T, int Tp,
                    const float* mean, const float* invstd, const float* gamma, int relu_in, unsigned short* dx,
                    size_t dx_bs, float* dgamma, float* dbeta, float* dbias, const void* sums_in, size_t sums_bytes,
                    void* ws, size_t ws_bytes, air_stream_t stream);
/* Res2 chain step (ecapa_tdnn.py:78-83): y1 = bf16(x * scale + shift); y2 = bf16(y1 + add) (add, y2 both or neither) */
int air_h_res2_bn_apply(const unsigned short* x, size_t x_bs, int B, int C, int T, int Tp, const float* scale,
                        const float* shift, unsigned short* y1, size_t y1_bs, const unsigned short* add, size_t add_bs,
                        unsigned short* y2, size_t y2_bs, air_stream_t stream);
/* SE gate + block residual (ecapa_tdnn.py:27-29,:93): out = bf16(x * sigmoid(z[b][c]) + res), and its backward
 * dx = bf16(dout * sigmoid(z)), dz = s (1 - s) sum_t dout x. */
int air_h_se_scale_fwd(const unsigned short* x, size_t x_bs, const float* z, const unsigned short* res, size_t res_bs,
                       int B, int C, int T, int Tp, unsigned short* out, size_t out_bs, air_stream_t stream);
int air_h_se_scale_bwd(const unsigned short* x, size_t x_bs, const float* z, const unsigned short* dout, size_t dout_bs,
                       int B, int C, int T, int Tp, unsigned short* dx, size_t dx_bs, float* dz, air_stream_t stream);
/* summed=True (ecapa_tdnn.py:163-166, "x2 = self.layer2(x + x1)"): air_h_se_scale_fwd with a second output, the running
 * sum of the block inputs, from the same pass - out as above (the same bits), sum = bf16(out + res) on the STORED out
 * (the bf16 + bf16 add of the reference under autocast).  sum: rows or a channel slice, distinct from x / res / out.
 * AIR_EINVAL for rows beyond the register cache (Tp > 2048), like every row kernel here. */
int air_h_se_scale_fwd_sum(const unsigned short* x, size_t x_bs, const float* z, const unsigned short* res, size_t res_bs,
                           int B, int C, int T, int Tp, unsigned short* out, size_t out_bs, unsigned short* sum,
                           size_t sum_bs, air_stream_t stream);
/* out = bf16(a + b), frames >= T zero: the gradient joins of summed=True (the backward of :163-166's adds: d x_k = its
 * slice of the concat gradient + d(x + x1 [+ x2])).  a, b, out: rows or channel slices; out may be a or b itself
 * (element for element, the same batch stride); any other overlap of out's address range with an operand's is refused
 * (AIR_EINVAL), as is Tp > 2048. */
int air_h_add(const unsigned short* a, size_t a_bs, const unsigned short* b, size_t b_bs, int B, int C, int T, int Tp,
              unsigned short* out, size_t out_bs, air_stream_t stream);
/* Context statistics (ecapa_tdnn.py:178) of a dense bf16 tensor and their backward folded into dx
 * (dx = bf16(dx + ...), ReLU mask of layer4's output, rowsum of the stored values): air_row_stats[_bwd]. */
int air_h_row_stats(const unsigned short* x, int B, int C, int T, int Tp, float* mean, float* std_or_null,
                    float clamp_min, air_stream_t stream);
int air_h_row_stats_bwd(const unsigned short* x, int B, int C, int T, int Tp, const float* mean, const float* std_,
                        const float* dmean, const float* dstd, float clamp_min, unsigned short* dx, int accumulate,
                        int relu_mask, float* rowsum_or_null, air_stream_t stream);
/* context=False (ecapa_tdnn.py:179-180, "global_x = x"): no statistics feed attention.0, so the backward of layer4's
 * ReLU (:173) is the mask alone - dx = bf16(dx) where x > 0, else 0, in place, and rowsum (B * C, may be NULL) = sum_t
 * of the stored dx: the bits of air_h_row_stats_bwd(accumulate = 1, relu_mask = 1) with zero dmean / dstd, without
 * reading mean / std.  x, dx: rows or channel slices, distinct.  AIR_EINVAL for Tp > 2048. */
int air_h_relu_mask_rowsum(const unsigned short* x, size_t x_bs, int B, int C, int T, int Tp, unsigned short* dx,
                           size_t dx_bs, float* rowsum_or_null, air_stream_t stream);
/* Attentive statistics pooling (ecapa_tdnn.py:143-185): logits (bf16) -> w = bf16(softmax_T) in place; [mu | sg]
 * from the STORED w.  bwd: dx written (bf16), w overwritten with bf16(d logits), rowsum of the stored d logits. */
int air_h_asp_fwd(const unsigned short* x, unsigned short* logits_to_w, int B, int C, int T, int Tp, float* out,
                  air_stream_t stream);
int air_h_asp_bwd(const unsigned short* x, unsigned short* w_to_dlogits, int B, int C, int T, int Tp, const float* out,
                  const float* dout, unsigned short* dx, float* rowsum_or_null, air_stream_t stream);
/* Edges of the bf16 region: rows -> dense (B, C, T) fp32; rows -> rows (channel-slice copies). */
int air_h_to_f32(const unsigned short* x, size_t x_bs, int B, int C, int T, int Tp, float* y, air_stream_t stream);
int air_h_copy(const unsigned short* x, size_t x_bs, int B, int C, int Tp, unsigned short* y, size_t y_bs,
               air_stream_t stream);
/* The K = 5 first layer (ecapa_tdnn.py:111) as a pointwise GEMM: dense fp32 (B, Cin, T) -> bf16 rows (B, rows, Tp),
 * row ci K + k = x[ci][t + k dil - pad] (zeros outside [0, T), behind T, and in rows >= Cin K), so that
 * air_h_conv1d_pointwise / air_h_conv1d_wgrad with the (Cout, Cin, K) weight seen as (Cout, Cin K [+ zero columns])
 * are the layer's forward and weight gradient. */
int air_h_unfold(const float* x, size_t x_bs, int B, int Cin, int T, int Tp, int K, int dil, int pad, int rows,
                 unsigned short* y, size_t y_bs, air_stream_t stream);

/* ----------------------------------------------------------------- LCNN ---
 * model.LCNN (model.py:511-610), the reference's default --model.  Its convolutions conv2 .. conv9 run on
 * air_conv2d_fwd_pre / _dgrad_pre / _wgrad (bias-free; conv3 / conv4's 96 outputs on weights zero-padded to 128
 * rows), its BatchNorm2d(affine=False) on the BatchNorm kernels with unit scale and zero shift, its Linear layers on
 * air_linear_*.  The kernels below are the rest.  Route byte of every post-MFM (post-pool) element: bits 0-1 the
 * winning 2x2 window position (dy * 2 + dx; 0 without pooling), bit 2 the Max-Feature-Map half (0: channel c, 1:
 * channel c + C/2).  Ties go to the first candidate, as torch's max(dim) / max_pool2d send the gradient. */
/* conv1 (model.py:528-530): Conv2d(1, 64, 5, pad 2) + bias -> MaxFeatureMap2D -> MaxPool2d(2, 2) in one pass.
 * x (B, 1, H, W), w (64, 1, 5, 5), bias (64); y and route (B, 32, H/2, W/2).  The 64 x H x W map is never written. */
int air_lcnn_conv1_fwd(const float* x, const float* w, const float* bias, int B, int H, int W, float* y,
                       uint8_t* route, air_stream_t stream);
/* conv1's weight (64, 25) and bias (64) gradients from the pooled gradient dy (B, 32, H/2, W/2) and the route bytes
 * (no data gradient: the input is features).  Deterministic (fixed-order reduction). */
size_t air_lcnn_conv1_wgrad_ws_bytes(void);
int air_lcnn_conv1_wgrad(const float* x, const float* dy, const uint8_t* route, int B, int H, int W, float* dw,
                         float* db, void* ws, size_t ws_bytes, air_stream_t stream);
/* MaxFeatureMap2D (model.py:512-545) of x + bias over channels [0, C) of x (B, Ctot, H, W), then with pool != 0
 * MaxPool2d(2, 2) (floor mode: an odd last row / column is dropped): y, route (B, C/2, Ho, Wo).  bias (C) may be
 * NULL (the conv's bias folded in here: model.py:531-563 convs all have one). */
int air_mfm_pool_fwd(const float* x, const float* bias, int B, int Ctot, int C, int H, int W, int pool, float* y,
                     uint8_t* route, air_stream_t stream);
/* The route backward: dx (B, Ctot, H, W) = dy where the element won its pair and window, 0 elsewhere (losers,
 * dropped rows / columns, padded channels [C, Ctot)). */
int air_mfm_pool_bwd(const float* dy, const uint8_t* route, int B, int Ctot, int C, int H, int W, int pool, float* dx,
                     air_stream_t stream);
/* The conv bias gradient behind an MFM: db[ch] (C) = sum of dy (B, C/2, S) over the positions channel ch won.
 * Deterministic. */
size_t air_mfm_bias_grad_ws_bytes(int C);
int air_mfm_bias_grad(const float* dy, const uint8_t* route, int B, int C, int S, float* db, void* ws, size_t ws_bytes,
                      air_stream_t stream);
/* dst[i] = src[i] for i < min(n_dst, n_src), 0 beyond n_src: zero-padded weight rows and the gradient rows copied back. */
int air_copy_pad(float* dst, size_t n_dst, const float* src, size_t n_src, air_stream_t stream);
/* y = a * b elementwise: nn.Dropout(0.7) of model.py:601 forward and backward with the keep-mask. */
int air_mul(const float* a, const float* b, size_t n, float* y, air_stream_t stream);
/* air_dropout_mask with the Philox offset held in DEVICE memory (read, then advanced by ceil(n / 4) behind the
 * draw), like air_randn_ctr: a captured hipGraph draws a fresh mask on every replay.  Same draw body as
 * air_dropout_mask (adv_head.hip).  counter: 8-byte aligned. */
int air_dropout_mask_ctr(float* keep, size_t n, float p, uint64_t seed, uint64_t* counter, air_stream_t stream);

/* ------------------------------------------- fused adversarial heads ------
 * All channel-classifier heads of one phase of the --ADV_AUG step in one call (csrc/adv_head.hip): per head k
 * GRL -> Linear(D, D/2) -> Dropout(p) -> ReLU -> Linear(D/2, C_k) -> ReLU (model.py:976-1023), the mean cross-entropy
 * and the accuracy count of main_train.py:381-387 / :426-432, and the backward of :394-402 / :441-453:
 *   h = relu(keep * (w1 x + b1)),  o = relu(w2 h + b2),  loss_k = mean_b CE(o_b, targets_b),
 *   correct_k = #(first argmax == target)   (a row of zeros predicts class 0, as air_softmax_ce_fwd),
 *   grads = [dw1 (H, D) | db1 (H) | dw2 (C, H) | db2 (C)] of loss_k, written (not accumulated), H = D / 2,
 *   dx (want_dx) = t_0 + t_1 + ... in head order, t_k = -lambda * d loss_k / d feats (lambda multiplied in last).
 * One workgroup per head; with several heads and want_dx a second launch adds the heads' terms.  Fixed summation
 * order, no floating-point atomics: the same inputs give the same bits.  Softmax and CE are the arithmetic of
 * air_softmax_ce_fwd / _bwd.
 * Dropout: `keep` (B, H), already scaled, is used as given; else with p > 0 and a `counter` (8-byte aligned device
 * uint64, one per head, not shared between heads) the mask is air_dropout_mask_ctr's draw - Philox(seed, *counter + quad)
 * over the flattened (B, H) mask - and the call advances the counter by (B * H + 3) / 4; else there is no mask (eval).
 * run_correct (optional, device int64): correct_k is added to it.
 * ws: air_adv_heads_ws_bytes(B, D, nheads, C, want_dx) bytes of device scratch (0 = unsupported arguments).
 * Supported: 1 <= B <= 4096; D even, 2 <= D <= 1024; 1 <= C_k <= 256; 1 <= nheads <= 4; 0 <= p < 1.  Anything else, a
 * NULL pointer, a short workspace or a misaligned / shared counter: AIR_EINVAL, ahead of any HIP call. */
#define AIR_ADV_MAX_HEADS 4
typedef struct AirAdvHead {
  const float* w1;             /* (H, D) */
  const float* b1;             /* (H) */
  const float* w2;             /* (C, H) */
  const float* b2;             /* (C) */
  const long long* targets;    /* (B) int64 */
  const float* keep;           /* (B, H) explicit scaled keep mask, or NULL */
  uint64_t* counter;           /* device Philox offset, or NULL */
  uint64_t seed;
  float* grads;                /* H*D + H + C*H + C floats */
  float* loss;                 /* device scalar */
  int* correct;                /* device scalar */
  long long* run_correct;      /* device scalar, or NULL */
  int C;
  float p;
} AirAdvHead;
typedef struct AirAdvHeads {
  int B, D, nheads, want_dx;
  float lambda;
  const float* feats;          /* (B, D) */
  float* dx;                   /* (B, D) when want_dx */
  void* ws;
  size_t ws_bytes;
  AirAdvHead head[AIR_ADV_MAX_HEADS];
} AirAdvHeads;
size_t air_adv_heads_ws_bytes(int B, int D, int nheads, const int* C, int want_dx);
int air_adv_heads(const AirAdvHeads* d, air_stream_t stream);

/* -------------------------------------------------------------- Res2Net ---
 * model.Res2Net(SEBottle2neck, [3, 4, 6, 3], baseWidth=26, scale=4) (model.py:256-509, main_train.py:169-170).
 * Its BatchNorms run on the BatchNorm kernels, the SE squeeze and the global average pool on air_row_stats, the SE
 * and cls_layer Linear layers on air_linear_*, the 1x1 layers whose shape the generic kernels accept (Cin % 8 == 0,
 * Cout % 64 == 0) on air_conv2d_*.  The kernels below are the rest. */
/* Narrow-channel convolution (csrc/conv_narrow.hip): 3x3 pad 1 at stride 1 or 2, or 1x1 stride 1; 1 <= Cin, Cout
 * <= 256 (AIR_EUNSUPPORTED beyond); Ho / Wo as PyTorch's.  x (B, Cin, H, W) and y (B, Cout, Ho, Wo) are NCHW with a
 * dense (C, H, W) block and a batch stride in elements (0 = dense): channel slices of wider tensors (the Res2
 * split / concat of model.py:459-476) are read and written in place.  The data / weight gradients take dx and dy in
 * the same layout (x_bstride for x / dx, y_bstride for y / dy). */
typedef struct {
  int B, Cin, H, W, Cout, K, stride, Ho, Wo;
  size_t x_bstride, y_bstride;
} AirConvNarrow;
/* y = conv(act(x), w); act = x*in_scale[ci] + in_shift[ci] (+ ReLU when relu != 0) when in_scale / in_shift are
 * set (a BatchNorm-apply + ReLU prologue; the zero padding is not activated), identity when both are NULL. */
int air_conv_narrow_fwd(const AirConvNarrow* p, const float* x, const float* w, const float* in_scale,
                        const float* in_shift, int relu, float* y, air_stream_t stream);
/* dx (=, or += when accumulate != 0) gradient with respect to the convolution's input (the activated input when the
 * forward had a prologue). */
int air_conv_narrow_dgrad(const AirConvNarrow* p, const float* dy, const float* w, float* dx, int accumulate,
                          air_stream_t stream);
/* dw (Cout, Cin, K, K) from x (with the same optional prologue as the forward) and dy.  Per-chunk partials in ws,
 * summed in chunk order: deterministic.  ws_bytes: air_conv_narrow_wgrad_ws_bytes (0 = unsupported shape). */
size_t air_conv_narrow_wgrad_ws_bytes(const AirConvNarrow* p);
int air_conv_narrow_wgrad(const AirConvNarrow* p, const float* x, const float* dy, const float* in_scale,
                          const float* in_shift, int relu, float* dw, void* ws, size_t ws_bytes, air_stream_t stream);
/* Res2 chain step with the ReLU of model.py:466: v = relu(x*scale[c] + shift[c]) written to y1 (a channel slice of
 * the concat); optional y2 = v + add (dense), the next branch's input "sp + spx[i+1]" (:463).  x, y1 and add are
 * (B, C, S) with a batch stride in floats (0 = dense); add and y2 both NULL or both set.  air_res2_bn_apply
 * (ECAPA's order, no ReLU) is unchanged. */
int air_res2_bn_relu_apply(const float* x, size_t x_bstride, int B, int C, int S, const float* scale,
                           const float* shift, float* y1, size_t y1_bstride, const float* add, size_t add_bstride,
                           float* y2, air_stream_t stream);
/* nn.AvgPool2d(k, stride, pad, ceil_mode, count_include_pad) on (B, C, H, W) channel slices (batch strides in floats,
 * 0 = dense), PyTorch's windows and divisors: the stage block's 3x3 pool of its last split (model.py:442,
 * count_include_pad) and the downsample's 2x2 ceil-mode pool (:294-298, count_include_pad=False).  Ho / Wo must be
 * PyTorch's output size.  The backward gathers each input's windows in the order PyTorch adds them; accumulate != 0
 * adds to dx. */
int air_avgpool2d_fwd(const float* x, size_t x_bstride, int B, int C, int H, int W, int k, int stride, int pad,
                      int ceil_mode, int count_include_pad, int Ho, int Wo, float* y, size_t y_bstride,
                      air_stream_t stream);
int air_avgpool2d_bwd(const float* dy, size_t dy_bstride, int B, int C, int H, int W, int k, int stride, int pad,
                      int ceil_mode, int count_include_pad, int Ho, int Wo, float* dx, size_t dx_bstride,
                      int accumulate, air_stream_t stream);
/* SE tail of a block (model.py:480-487, :504-505): out = relu(x*sigmoid(z[b][c]) + res), all (B, C, S) dense.
 * bwd: with dpre = dout where out > 0: dx = dpre*sigmoid(z), dres = dpre (NULL: not written), dz[b][c] =
 * sigmoid'(z) sum_s dpre*x (one workgroup per row, fixed order).  air_se_scale_* (ECAPA, no ReLU) is unchanged. */
int air_se_relu_fwd(const float* x, const float* z, const float* res, int B, int C, int S, float* out,
                    air_stream_t stream);
int air_se_relu_bwd(const float* x, const float* z, const float* out, const float* dout, int B, int C, int S,
                    float* dx, float* dz, float* dres, air_stream_t stream);
/* F.log_softmax(z, dim=-1) of the (B, C) logits (model.py:353) and its backward dz = dout - exp(out) sum_c dout. */
int air_log_softmax_fwd(const float* z, int B, int C, float* out, air_stream_t stream);
int air_log_softmax_bwd(const float* out, const float* dout, int B, int C, float* dz, air_stream_t stream);

/* ----------------------------------------------------------- OC-Softmax ---
 * AngularIsoLoss.forward == OCSoftmax.forward (loss.py:73-97, :187-206).
 * x (B,D), center (1,D), labels (B,) int64.  loss: scalar; neg_scores (B,).
 * bwd: dx (B,D), dcenter (1,D) for d(loss*gscale).
 * One workgroup each (the loss is summed in a fixed order): B <= 4096, else AIR_EUNSUPPORTED.
 */
int air_ocsoftmax_fwd(const float* x, const float* center, const int64_t* labels, int B, int D,
                      float r_real, float r_fake, float alpha, float* loss, float* neg_scores,
                      air_stream_t stream);
int air_ocsoftmax_bwd(const float* x, const float* center, const int64_t* labels, int B, int D,
                      float r_real, float r_fake, float alpha, const float* gscale_dev,
                      float* dx, float* dcenter, air_stream_t stream);

/* ------------------------------------------------- other loss heads ---
 * csrc/loss_heads.hip.  One workgroup each, per-row terms summed in a fixed order (no atomics: deterministic);
 * x (B,D) fp32, labels (B,) int64, B <= 4096, else AIR_EUNSUPPORTED.  bwd: gradients of loss * gscale
 * (gscale_dev: device scalar or NULL for 1).
 *
 * P2SGradLoss.forward (loss.py:300-335): w = weight.renorm(2, 1, 1e-5).mul(1e5) (weight (D,C), C <= 4,
 * D <= 1024), cos = clamp(x w / |x|, -1, 1) with no epsilon on |x| (:314-325), target = one-hot smoothed by
 * `smooth` (:291-297, :331), loss = MSE(cos, target) averaged over B x C (:333); neg_cos0 = -cos[:, 0] (:335).
 * bwd: dx (B,D) and dweight (D,C) through renorm as torch autograd differentiates it (scale and column-norm
 * term); clamp passes the gradient where -1 <= cos <= 1. */
int air_p2sgrad_fwd(const float* x, const float* weight, const int64_t* labels, int B, int D, int C, float smooth,
                    float* loss, float* neg_cos0, air_stream_t stream);
int air_p2sgrad_bwd(const float* x, const float* weight, const int64_t* labels, int B, int D, int C, float smooth,
                    const float* gscale_dev, float* dx, float* dweight, air_stream_t stream);
/* IsolateLoss.forward (loss.py:119-139): relu(|x - c| - r_real) averaged over the label-0 rows plus
 * relu(r_fake - |x - c|) averaged over the label-1 rows; square != 0: IsolateSquareLoss (:155-173), squared norms
 * with r_real, r_fake passed ALREADY SQUARED.  A class without rows gives NaN (torch's mean of an empty tensor).
 * center (1,D).  dist_or_null: (B,) |x - c| (main_train.py:548's dev-pass score) or NULL.
 * bwd: dx (B,D), dcenter (1,D); the norm's gradient is 0 at |x - c| == 0 and a ReLU input of 0 passes none. */
int air_isolate_fwd(const float* x, const float* center, const int64_t* labels, int B, int D, float r_real,
                    float r_fake, int square, float* loss, float* dist_or_null, air_stream_t stream);
int air_isolate_bwd(const float* x, const float* center, const int64_t* labels, int B, int D, float r_real,
                    float r_fake, int square, const float* gscale_dev, float* dx, float* dcenter,
                    air_stream_t stream);
/* AMSoftmax.forward (loss.py:217-234), forward only: logits (B,C) = cosine of the rows of x and of centers (C,D),
 * no epsilon; margin_logits = s * (logits - m * onehot(labels)). */
int air_amsoftmax_fwd(const float* x, const float* centers, const int64_t* labels, int B, int D, int C, float s,
                      float m, float* logits, float* margin_logits, air_stream_t stream);

/* --------------------------------------------------- evaluation metrics ---
 * The two minima the reference reads off the DET curve of a dev / eval pass, exactly, without leaving the stream:
 * the EER point of compute_eer (eval_metrics.py:19-46: mergesort, cumsum, argmin |frr - far|; called on both score
 * polarities at main_train.py:662-664) and the min t-DCF point (the argmin of evaluate_tDCF_asvspoof19.py:58-59 over
 * the curve of compute_tDCF, eval_metrics.py:157-172) - for all trials and, from the same sort, for each group of a
 * breakdown by attack or by channel condition.  scores: n fp32; labels: n integers of label_bytes (4 | 8) bytes,
 * 0 = bona fide, anything else = spoof; negate != 0 evaluates -scores.  n <= air_eval_max_trials() (2^20), more:
 * AIR_EUNSUPPORTED.  No allocation, no host synchronisation: all scratch is the caller's workspace (16-byte aligned),
 * everything is enqueued on `stream`.
 *
 * Groups (air_eval_det_min_grouped): groups holds n integers of group_bytes (4 | 8) bytes.  g in 0 .. n_groups-1: the
 * trial belongs to group g; g == -1: the trial belongs to EVERY group (per-attack tables: bona fide trials -1, spoof
 * trials their attack; per-channel tables: every trial its condition).  Any other id belongs to no group and is
 * counted into recs[0].reserved[0]: the caller must refuse the result.  1 <= n_groups <= air_eval_max_groups() (128),
 * otherwise AIR_EUNSUPPORTED.  air_eval_det_min is the same chain without groups: one record, reserved[0] = 0.
 *
 * Per trial one 64-bit key, (order-preserving image of the score) << 9 | is_spoof << 8 | code with -0.0 taken as +0.0
 * and code = g + 1 (0: every group - every trial of a call without groups; 255: none).  The keys are padded with
 * all-ones sentinels to a power of two >= air_eval_sort_block() and sorted ascending by a bitonic network, ONCE per
 * call whatever n_groups is: the group rides below the class bit, so "bona fide first among equal scores" holds inside
 * every subset.  Then per sort block the class / NaN / inf counts of every record (a histogram of the codes), an
 * exclusive prefix over the blocks per record, and the curve walk: per record the scan of "member and spoof" / "member
 * and bona fide" over the sorted keys gives rejected_non[k] and rejected_tar[k] after the record's k lowest members,
 * k = 0 .. its size; in fp64, frr = rejected_tar / n_tar, far = (n_non - rejected_non) / n_non from the record's own
 * counts, and the record gets the FIRST k that minimises |frr - far| and, with want_dcf, the FIRST k that minimises
 * (c1 * frr + c2 * far) / min(c1, c2) (c1, c2: the C1, C2 of eval_metrics.py:160-162, computed by the caller), and its
 * distinct scores (a member counts when the member before it has another score).  Integer atomics only (counts and
 * the index of a block's last member), fixed-order reductions; every word of a record is written by the call.
 *
 * recs holds n_groups + 1 records.  recs[0] is the pooled record: every trial is a member.  recs[1 + g] is, field for
 * field, the record the chain writes when it is given the trials of {i : g_i == g or g_i == -1} alone: n_tar, n_non,
 * n_nan, n_inf, n_distinct of that subset, eer_idx / dcf_idx as the index on the subset's OWN curve (members rejected
 * so far), *_rej_non the spoof members among them, *_score_first the subset's lowest score, *_score_at the score of its
 * k-th lowest member.  A group without members has all-zero counts and 0.0 scores.  The caller finishes on the host
 * from the integer counts; it must refuse n_nan > 0 (numpy sorts NaN last) and an empty class (the indices are then
 * meaningless). */
typedef struct air_eval_record {
  uint32_t n_tar, n_non;          /* bona fide / spoof trials */
  uint32_t n_nan, n_inf;          /* NaN / +-inf scores (compute_tDCF refuses both, eval_metrics.py:147-149) */
  uint32_t n_distinct;            /* distinct scores (compute_tDCF refuses < 3, eval_metrics.py:152-154) */
  uint32_t has_dcf;               /* the dcf_* fields are valid */
  uint32_t eer_idx, eer_rej_non;  /* k of the EER point, rejected_non[k] */
  float eer_score_first;          /* sorted score 0 */
  float eer_score_at;             /* sorted score k - 1 (score 0 when k = 0) */
  uint32_t dcf_idx, dcf_rej_non;
  float dcf_score_first, dcf_score_at;
  uint32_t reserved[2];
} air_eval_record; /* 64 bytes */
int air_eval_max_trials(void);
int air_eval_sort_block(void); /* keys sorted per workgroup in LDS: the block boundary of the network */
int air_eval_max_groups(void);
/* Workspace bytes without groups and with 1 .. air_eval_max_groups() of them; 0: an argument out of range. */
size_t air_eval_workspace_bytes(int n);
size_t air_eval_workspace_bytes_grouped(int n, int n_groups);
/* The whole chain, pooled: keys, sort, curve minima into one record.  c1, c2 are read only with want_dcf. */
int air_eval_det_min(const float* scores, const void* labels, int label_bytes, int n, int negate, int want_dcf,
                     double c1, double c2, air_eval_record* rec, void* ws, size_t ws_bytes, air_stream_t stream);
/* The whole chain with groups.  The t-DCF weights are per record: c12_dev points to (n_groups + 1) x {c1, c2} doubles
 * in DEVICE memory (row 0 pooled, row 1 + g group g; per-attack t-DCF has a C2 per attack) and is read only with
 * want_dcf (NULL otherwise). */
int air_eval_det_min_grouped(const float* scores, const void* labels, int label_bytes, const void* groups,
                             int group_bytes, int n, int n_groups, int negate, int want_dcf, const double* c12_dev,
                             air_eval_record* recs, void* ws, size_t ws_bytes, air_stream_t stream);
/* The three steps of air_eval_det_min on the same workspace (the keys are its first npad * 8 bytes): air_eval_keys
 * builds the padded keys; air_eval_sort_keys sorts them (np.sort of the keys, eval_metrics.py:26 up to the order of
 * equal keys); air_eval_curve_min needs only the sorted keys and writes the whole record. */
int air_eval_keys(const float* scores, const void* labels, int label_bytes, int n, int negate, void* ws, size_t ws_bytes,
                  air_stream_t stream);
int air_eval_sort_keys(int n, void* ws, size_t ws_bytes, air_stream_t stream);
int air_eval_curve_min(int n, int want_dcf, double c1, double c2, air_eval_record* rec, void* ws, size_t ws_bytes,
                       air_stream_t stream);

/* -------------------------------------------------------- score fusion ---
 * The fusion of the scores of K systems as the reference's score_fusion.py computes it with pandas: out[n] = the sum
 * (mode 0: avg_fuse, score_fusion.py:21-28) or the mean over the systems that have the trial (mode 1: weighted_fuse,
 * :31-43) of weights[k] * score of trial n in system k, k = 0 .. K-1 in that order, as a compensated (Kahan) fp32
 * accumulation: v = score * weight rounded to fp32 on its own (no product without weights); y = v - c; t = s + y;
 * c = (t - s) - y, reset to 0 where it is NaN (an infinite term); s = t - every step one correctly rounded fp32
 * operation, never contracted.  A NaN v is skipped and not counted.  The mean is s / (float)count, one fp32 division.
 *
 * scores: K rows, system-major, row k at scores + k * row_stride.  index NULL (aligned): trial n is element n of every
 * row (coalesced reads; row_stride >= N for K > 1).  index (K x N int32, device): index[k * N + n] is the position of
 * trial n in row k, negative = system k does not have it (a gather); positions must lie in [0, row_stride), anything
 * else counts as absent and is never dereferenced.  weights: K fp32 in DEVICE memory (a captured graph replays with new
 * weights) or NULL.  n_present (N uint32 or NULL) gets the number of terms counted; a trial without any gets NaN and 0
 * (pandas has no such row; its sum over a group whose every score is NaN is 0.0 - here NaN as well).
 * N = 0: nothing is launched.  AIR_EINVAL: K < 1, N < 0, a mode other than 0 | 1, scores or out NULL, a row_stride
 * below the row, out overlapping the K rows; AIR_EUNSUPPORTED: K > air_score_fuse_max_systems(), N or row_stride above
 * 2^38 - all ahead of any HIP call, out untouched. */
int air_score_fuse_max_systems(void); /* 64 */
int air_score_fuse(const float* scores, int64_t row_stride, const int32_t* index, const float* weights, int K, int64_t N,
                   int mode, float* out, uint32_t* n_present, air_stream_t stream);

/* ------------------------------------------------ embedding projections ---
 * What the reference's visualize.py asks of scikit-learn, on the device (csrc/embed_vis.hip): PCA without its
 * eigensolver, and exact t-SNE - TSNE(method="exact") - in two output dimensions with the Euclidean metric.
 * LIMITS: 2 <= N <= 16384 rows (air_vis_max_n), 1 <= D <= 1024 features (air_vis_max_d), at most 16 principal components
 * (air_pca_max_components).  Outside them (N < 2 included) the size queries return 0 and the calls AIR_EUNSUPPORTED
 * (AIR_EINVAL for D < 1 or a NULL pointer).  Workspaces are the caller's, 16-byte aligned (AIR_EWORKSPACE when too small); nothing
 * is allocated or synchronised.  All sums are fixed-order partial sums in fp64 - no floating-point atomics: two calls
 * on one input return the same bits.
 *
 * air_pca_gram: mean[d] = the column means of x (N, D) fp32, and gram (D x D fp64, symmetric to the bit) =
 * sum_n (x[n] - mean)(x[n] - mean)^T - two passes, the centred differences in fp32, products and sums in fp64.  The
 * host takes the eigenvectors (numpy.linalg.eigh).  air_pca_project: out (N, K) fp32 = (x - mean) comps^T for comps
 * (K, D) fp32.
 * air_pairwise_sqdist: out (N, N) fp32 = sum_k (x_i[k] - x_j[k])^2 in feature order - never the expansion
 * |x_i|^2 + |x_j|^2 - 2 x_i.x_j; the diagonal and equal rows give exactly 0, out[i][j] and out[j][i] the same bits.
 * air_tsne_affinities: scikit-learn's _binary_search_perplexity over dist (N, N) fp32: cond (N, N) fp32 gets the
 * conditional probabilities (diagonal 0), beta (N) fp32 each row's precision.  fp64 inside, at most 100 bisection steps,
 * tolerance 1e-5 nats, a zero row sum replaced by 1e-8.  cond must not alias dist.
 * air_tsne_joint: P (N, N) in place: max((C + C^T) / max(sum(C + C^T), eps), eps) off the diagonal, 0 on it,
 * eps = 2.220446049250313e-16 (_joint_probabilities); symmetric to the bit.  ws: air_tsne_ws_bytes(N).
 *
 * The descent, one iteration = air_tsne_pairs + air_tsne_update (+ air_tsne_check), all on ws of air_tsne_ws_bytes(N):
 * air_tsne_pairs: the passes over the pairs of the embedding y (N, 2) fp32, in fp64: Z = sum n_ij,
 *   n_ij = 1 / (1 + |y_i - y_j|^2), from y alone; then, reading P once (the JOINT distribution: symmetric - row i is
 *   read as column i), per row and column split the sum of (e p_ij - q_ij) n_ij (y_i - y_j), q_ij = max(n_ij / Z, eps),
 *   e = exaggeration - _kl_divergence's terms with its floor of q.  want_kl: one more pass for
 *   sum p log(max(p, eps) / q), p = e p_ij.
 * air_tsne_gradient: grad (N, 2) fp32 = 4 x the row sums of the last air_tsne_pairs.
 * air_tsne_update: _gradient_descent's step from the same partials: gains += 0.2 where update * grad < 0, *= 0.8
 *   elsewhere, floored at 0.01; update = momentum * update - learning_rate * gains * grad; y += update.
 * air_tsne_check: behind the update of iteration `iter`: writes kl (NaN unless have_kl), grad_norm (of gains * grad, as
 *   scikit-learn takes it) and n_iter = iter into the status record, and with apply_rules stops the run when the KL
 *   has not improved for more than n_iter_without_progress iterations or grad_norm <= min_grad_norm.
 * air_tsne_begin: the start of a _gradient_descent call at iteration iter: update = 0, gains = 1, best error forgotten;
 *   first != 0 initialises the record too.
 * Once the record says stopped, pairs / update / check / begin (first = 0) return without touching anything.
 * air_tsne_run enqueues the whole schedule: begin(first); per iteration i < max_iter: momentum 0.5 and
 * early_exaggeration while i < exploration_iter, then begin(i) once, momentum 0.8, exaggeration 1 and a check every
 * n_iter_check iterations; the KL is also taken at the last iteration.  The first phase always runs its full length. */
typedef struct {
  int stopped;       /* 0 | 1 */
  int reason;        /* 0 running / ran to max_iter, 1 no progress, 2 gradient norm */
  int n_iter;        /* the last iteration a check ran behind (scikit-learn's n_iter_) */
  int best_iter;
  double best_error;
  double kl;
  double grad_norm;
  double pad[3];
} air_tsne_status; /* 64 bytes, device memory */
typedef struct {
  int max_iter, exploration_iter, n_iter_check, n_iter_without_progress;
  float learning_rate, early_exaggeration;
  double min_grad_norm;
} air_tsne_schedule;
int air_vis_max_n(void);              /* 16384 */
int air_vis_max_d(void);              /* 1024 */
int air_pca_max_components(void);     /* 16 */
size_t air_pca_ws_bytes(int N, int D);
size_t air_tsne_ws_bytes(int N);
int air_pca_gram(const float* x, int N, int D, float* mean, double* gram, void* ws, size_t ws_bytes, air_stream_t stream);
int air_pca_project(const float* x, int N, int D, const float* mean, const float* comps, int K, float* out,
                    air_stream_t stream);
int air_pairwise_sqdist(const float* x, int N, int D, float* out, air_stream_t stream);
int air_tsne_affinities(const float* dist, int N, float perplexity, float* cond, float* beta, air_stream_t stream);
int air_tsne_joint(float* P, int N, void* ws, size_t ws_bytes, air_stream_t stream);
int air_tsne_begin(float* update, float* gains, int N, int iter, int first, air_tsne_status* status, air_stream_t stream);
int air_tsne_pairs(const float* P, const float* y, int N, float exaggeration, int want_kl, const air_tsne_status* status,
                   void* ws, size_t ws_bytes, air_stream_t stream);
int air_tsne_gradient(int N, float* grad, void* ws, size_t ws_bytes, air_stream_t stream);
int air_tsne_update(float* y, float* update, float* gains, int N, float momentum, float learning_rate,
                    const air_tsne_status* status, void* ws, size_t ws_bytes, air_stream_t stream);
int air_tsne_check(int N, int iter, int have_kl, int apply_rules, int n_iter_without_progress, double min_grad_norm,
                   air_tsne_status* status, void* ws, size_t ws_bytes, air_stream_t stream);
int air_tsne_run(const float* P, float* y, float* update, float* gains, int N, const air_tsne_schedule* schedule,
                 air_tsne_status* status, void* ws, size_t ws_bytes, air_stream_t stream);

/* ---------------------------------------------------------- FLAC decode ----
 * The waveform read of raw_dataset.py:20-28 (librosa.load / sf.read of a 16 kHz, 16-bit, mono .flac) for a batch of
 * B files at once, from their compressed audio frames to a ragged (B, Lcap) PCM batch.  The served format is the
 * fixed-block-size subset of RFC 9639, mono, 16 bit: CONSTANT / VERBATIM / FIXED 0..4 / LPC 1..32 subframes, wasted
 * bits, RICE and RICE2 residuals of every partition order with escape partitions, every block-size, sample-rate and
 * frame-number coding, header CRC-8 and frame CRC-16.  The arithmetic is integer: the samples are the encoder's.
 *
 * bytes: the audio frames of the B files (metadata stripped) in one buffer of total_bytes, 4-byte aligned.
 * byte_off (B + 1): row b occupies bytes [(byte_off[b] + 3) & ~3, byte_off[b + 1]) - every row starts 4-byte aligned
 * and ends at its exact last byte.  lengths (B): samples of row b (STREAMINFO total samples).  blocksize (B): the
 * row's STREAMINFO block size (every frame but the last has it, the last has it or fewer).
 * Output: y16 (B, Lcap) int16 and / or y32 (B, Lcap) fp32 = sample / 32768 (exact); at least one is non-NULL.  Samples
 * [lengths[b], Lcap) of every row are zeroed whatever its status.  status (B) int32: AIR_FLAC_OK or the first reason
 * row b could not be served; such a row's samples below lengths[b] are unspecified, every other row is unaffected.
 * Nothing is read outside [0, total_bytes), nothing is written outside the outputs, status and ws, whatever the
 * bitstream, byte_off, lengths or blocksize hold.
 *
 * Frames are located on the device (their lengths are not in their headers): every byte position that carries a
 * frame header consistent with the row (sync, valid codes, mono, 16 bit, block size <= the row's, CRC-8) is a
 * candidate; every candidate's bitstream is walked to its end offset and CRC-16; the chain from offset 0 through end
 * offsets must consist of candidates with matching CRC-16 and frame numbers 0, 1, 2 .., end at the row's last byte
 * and hold lengths[b] samples.  Only chain frames are decoded, so a sync pattern inside a payload never reaches
 * the output.  ws: air_flac_workspace_bytes(total_bytes, B) bytes, 16-byte aligned: one bit per byte position plus a
 * 16-byte record per candidate slot; two candidates are at least 5 bytes apart, the row's slots (a quarter of its
 * bytes) cannot run out for that reason - a row that would still need more gets AIR_FLAC_CANDIDATE_OVERFLOW. */
#define AIR_FLAC_OK 0
#define AIR_FLAC_LOST_SYNC 1          /* the chain of frames breaks, or stops short of the row's last byte */
#define AIR_FLAC_BAD_CRC16 2          /* a chain frame's CRC-16 does not match */
#define AIR_FLAC_UNSUPPORTED 3        /* a chain frame outside the served subset (stereo, other sample sizes, reserved
                                         codes, negative LPC shift, precision code 1111, variable block size) */
#define AIR_FLAC_LENGTH_MISMATCH 4    /* the chain holds another number of samples than lengths[b] (or > Lcap) */
#define AIR_FLAC_CANDIDATE_OVERFLOW 5 /* more candidates than the row's record slots */
size_t air_flac_workspace_bytes(size_t total_bytes, int B);
int air_flac_decode(const uint8_t* bytes, size_t total_bytes, const int* byte_off, const int* lengths,
                    const int* blocksize, int B, int Lcap, int16_t* y16_or_null, float* y32_or_null, int* status,
                    void* ws, size_t ws_bytes, air_stream_t stream);

/* ------------------------------------------------- WAV decode / resample ----
 * The waveform read of raw_dataset.py:20-28 for ``.wav`` files and for anything that is not at the target rate:
 * librosa.load(path, sr=16000) returns a mono float waveform at 16 kHz whatever the file's rate, channel count or sample
 * format.  One launch turns a packed batch of WAV payloads (air_wav_decode) or a dense ragged PCM batch
 * (air_resample_ragged) into the (B, Lcap_out) batch at the target rate; no host synchronisation, no workspace.
 *
 * The resampler is defined by its formulas (band-limited sinc interpolation with the parameters of resampy's
 * 'kaiser_best' filter, every coefficient evaluated exactly at its phase - no table-lookup quantisation):
 *   Z = 64, R = 0.9475937167399596, BETA = 14.769656459379492
 *   w(u) = I0(BETA sqrt(1 - (u / Z)^2)) / I0(BETA);  h(u) = R sinc(R u) w(u) for |u| < Z, else 0 (sinc(x) = sin(pi x) / (pi x))
 *   g = gcd(sr_in, sr_out), L = sr_out / g, M = sr_in / g, s = min(1, L / M), H = ceil(Z / s) (in integers), K = 2 H
 *   y[t] = sum_{j < K} c[p][j] x[n0 - H + 1 + j],  n0 = floor(t M / L), p = (t M) mod L (64 bit), x = 0 outside [0, n)
 *   c[p][j] = s h(s (p / L + H - 1 - j)), evaluated in fp64 and rounded once to fp32; n_out = ceil(n L / M).
 * The device accumulates in fp32: four interleaved ascending fmaf chains (j mod 4), summed (a0 + a1) + (a2 + a3).
 * sr_in == sr_out is the identity path: L = M = 1, K = 0, no table, no arithmetic beyond the format conversion.
 *
 * air_resample_geometry: AIR_EINVAL for a non-positive rate, L > AIR_RESAMPLE_MAX_L or K > AIR_RESAMPLE_MAX_K
 * (source rates above 16 x the target).  air_resample_table_host fills the L x K table (row p = phase p).  Neither
 * makes a HIP call.
 *
 * desc (host memory, read during the call): nrates <= AIR_RESAMPLE_MAX_RATES records {L, M, K, table_off}; tables
 * (device, fp32, table_elems values) holds record r's L x K table at table_off.  rate_idx (B, device): the record of
 * row b.  A desc with nrates outside [1, 8], L / K outside what air_resample_geometry allows, an odd K, an identity
 * record with K != 0 or a table outside [0, table_elems): AIR_EINVAL, as are NULL pointers, non-positive sizes and, for
 * air_resample_ragged, an in_kind other than AIR_PCM_S16 / AIR_PCM_F32 - all ahead of any HIP call.
 *
 * air_wav_decode: bytes / byte_off as air_flac_decode's (row b occupies [(byte_off[b] + 3) & ~3, byte_off[b + 1]):
 * the file's ``data`` payload, interleaved little-endian frames).  frames (B): frames of row b.  fmt (B):
 * AIR_WAV_FMT(kind, bytes per sample, channels).  Conversion to float is what a libsndfile float read returns:
 * u8 (v - 128) / 128, s16 v / 2^15, s24 v / 2^23, s32 v / 2^31, f32 as is, f64 rounded to fp32; C <= 8 channels are
 * summed in fp32 in channel order and divided once by C.  air_resample_ragged: x is (B, Lcap_in) int16 or fp32 mono,
 * lengths (B) its valid samples.
 * Output: y16 (B, Lcap_out) int16 = saturating round-half-even of 32768 y and / or y32 (B, Lcap_out) fp32 = y, from
 * the same accumulation; at least one is non-NULL.  Samples [n_out[b], Lcap_out) are zero.  status (B) int32.  A row
 * whose frames do not fit in its bytes (or lengths[b] > Lcap_in), or whose n_out exceeds Lcap_out:
 * AIR_WAV_LENGTH_MISMATCH; a format code outside the table above or a rate_idx outside desc: AIR_WAV_BAD_FORMAT.  Such
 * a row is all zeros; nothing is read outside the row or written outside the outputs; other rows are unaffected. */
#define AIR_RESAMPLE_MAX_L 640
#define AIR_RESAMPLE_MAX_K 2048
#define AIR_RESAMPLE_MAX_RATES 8
#define AIR_WAV_MAX_CHANNELS 8
#define AIR_PCM_U8 0
#define AIR_PCM_S16 1
#define AIR_PCM_S24 2
#define AIR_PCM_S32 3
#define AIR_PCM_F32 4
#define AIR_PCM_F64 5
#define AIR_WAV_FMT(kind, bytes, channels) ((kind) | ((bytes) << 4) | ((channels) << 8))
#define AIR_WAV_OK 0
#define AIR_WAV_LENGTH_MISMATCH 1
#define AIR_WAV_BAD_FORMAT 2
typedef struct {
  int L, M, K, table_off;
} air_resample_rate;
typedef struct {
  int nrates;
  air_resample_rate rate[AIR_RESAMPLE_MAX_RATES];
} air_resample_desc;
int air_resample_geometry(int sr_in, int sr_out, int* L, int* M, int* K);
int air_resample_table_host(int sr_in, int sr_out, float* table);
int air_resample_ragged(const void* x, int in_kind, int B, int Lcap_in, const int* lengths, const int* rate_idx,
                        const air_resample_desc* desc, const float* tables, size_t table_elems, int16_t* y16_or_null,
                        float* y32_or_null, int Lcap_out, int* status, air_stream_t stream);
int air_wav_decode(const uint8_t* bytes, size_t total_bytes, const int* byte_off, const int* frames, const int* fmt,
                   const int* rate_idx, int B, const air_resample_desc* desc, const float* tables, size_t table_elems,
                   int16_t* y16_or_null, float* y32_or_null, int Lcap_out, int* status, air_stream_t stream);

/* -------------------------------------------------------- device corpus ---
 * The decoded corpus held in HBM and the batch selection of main_train.py:226-345 on the device: a flat store of
 * utterances (int16 or fp32, every utterance starting at a multiple of 8 elements), a random permutation per flow and
 * epoch, and one gather per batch that also draws the crop offsets of dataset.py:69.  Nothing here allocates or
 * synchronises; everything is enqueued on `stream`.
 *
 * Random words.  word(i, s) is word 0 of the Philox4x32-10 block with counter {i, s, 0, 0} and key {seed lo, seed hi}
 * (the generator of air_dropout_mask / air_randn).  s = (generation << 2) | kind: kind 0 and 1 are the permutations of
 * the first and the second flow, kind 2 the crop offsets.  generation < 2^30.
 *
 * air_corpus_permutation: key_i = (uint64)word(i, stream_id) << 32 | i for i < n, padded with all-ones sentinels in the
 * layout air_eval_sort_keys sorts - the keys are the first npad * 8 bytes of the workspace, npad the power of two
 * >= max(n, air_eval_sort_block()) - sorted by air_eval_sort_keys itself; perm_out[j] = lo + (key_j & 0xffffffff).  The
 * keys are distinct, so perm_out is np.sort of the keys exactly.  1 <= n <= air_eval_max_trials() (2^20), more:
 * AIR_EUNSUPPORTED.  ws: 16-byte aligned, >= air_corpus_permutation_ws_bytes(n) (= air_eval_workspace_bytes(n)) bytes.
 *
 * air_corpus_copy_rows: rows ragged rows of elem_bytes (2 | 4) byte elements.  Row r is read at src + src_off[r]
 * (src_off NULL: r * src_stride) and written at dst + dst_off[r] (dst_off NULL: r * dst_stride), offsets and strides in
 * elements; min(max(lengths[r], 0), max_len) elements are copied.  dst_cap > 0 (needs dst_off NULL, max_len <= dst_cap
 * <= dst_stride): the elements [length, dst_cap) of every row are written as zeros.  One workgroup per row and tile of
 * air_corpus_copy_tile(elem_bytes) elements; a row whose two ends are 16-byte aligned moves 16 bytes per lane, any
 * other single elements.  The source is never read at or beyond a row's length.  rows <= 65535.
 *
 * air_corpus_gather: one batch of B = seg[0].count (+ seg[1].count) rows, those of seg[0] first.  Row r of a segment is
 * utterance u = perm[first + r] (perm NULL: first + r); a u outside [0, n) yields an empty row.  pcm (B, Lcap) gets the
 * utterance's samples through the copy above and zeros in [length, Lcap); lengths / labels / tags / index /
 * channels[b, 0 .. n_channels) the store's entries of u; start[b] the crop offset: T = 1 + length / hop, 0 when
 * T <= feat_len, else ((uint64)word(u, generation << 2 | 2) * (T - feat_len)) >> 32 - below T - feat_len, the exclusive
 * bound of np.random.randint(T - feat_len).  Lcap: a multiple of 8 and >= every length drawn (a longer utterance is
 * cut at Lcap; the caller knows the lengths and refuses it); pcm 16-byte aligned.  channels NULL exactly when the view
 * has none. */
typedef struct air_corpus_view {
  const void* samples;      /* the store, elem_bytes per sample */
  const int64_t* offsets;   /* n (+ 1) element offsets, each a multiple of 8 */
  const int* lengths;       /* n */
  const int64_t* labels;    /* n */
  const int64_t* tags;      /* n */
  const int64_t* index;     /* n */
  const int64_t* channels;  /* (n, n_channels) or NULL */
  int64_t n;
  int n_channels;
  int elem_bytes;           /* 2 | 4 */
} air_corpus_view;
typedef struct air_corpus_segment {
  const int64_t* perm;      /* device, or NULL: the identity */
  int64_t first;
  int count;
  uint32_t generation;      /* of the crop draws */
} air_corpus_segment;
int air_corpus_copy_tile(int elem_bytes); /* elements per workgroup tile; 0: unsupported element size */
size_t air_corpus_permutation_ws_bytes(int n);
int air_corpus_permutation(int64_t lo, int n, uint64_t seed, uint32_t stream_id, int64_t* perm_out, void* ws,
                           size_t ws_bytes, air_stream_t stream);
int air_corpus_copy_rows(const void* src, const int64_t* src_off, int64_t src_stride, void* dst, const int64_t* dst_off,
                         int64_t dst_stride, const int* lengths, int rows, int max_len, int dst_cap, int elem_bytes,
                         air_stream_t stream);
int air_corpus_gather(const air_corpus_view* c, const air_corpus_segment* seg, int nseg, uint64_t seed, int feat_len,
                      int hop, int Lcap, void* pcm, int* lengths, int64_t* labels, int64_t* tags, int64_t* channels,
                      int64_t* index, int* start, air_stream_t stream);

/* ---------------------------------------------------------- GMM back-end ---
 * A diagonal-covariance Gaussian mixture on feature frames: fp64 EM and log-likelihood scoring (the ASVspoof baselines
 * B01/B02 are two such models, bona fide and spoof, scored by the log-likelihood ratio).  No reference counterpart;
 * the arithmetic is scikit-learn 1.7's GaussianMixture(covariance_type="diag") from a given initialisation
 * (_estimate_log_gaussian_prob, _estimate_gaussian_covariances_diag, _m_step).  This block is the specification;
 * tests/gmm_oracle.py states it in numpy.
 *
 * A model is w (K), mu (K, D), var (K, D), all fp64.  Frames x are fp32 and are widened exactly.  With p = 1 / var:
 *
 *   lp[n,k]  = log w_k - 0.5 * (D log(2 pi) + sum_d mu^2 p + sum_d log var) + sum_d x (mu p) - 0.5 sum_d x^2 p
 *   lse[n]   = logsumexp_k lp[n,k]                (max-shifted)
 *   r[n,k]   = exp(lp[n,k] - lse[n])
 *   S0[k] = sum_n r    S1[k,d] = sum_n r x    S2[k,d] = sum_n r x^2    LL = sum_n lse    Nf = number of frames
 *   M-step:  nk = S0 + 10 * 2^-52;  mu = S1 / nk;  var = S2 / nk - mu^2 + reg_covar;  w = nk / sum_k nk;
 *            lower_bound = LL / Nf
 *
 * score_samples = lse; a row's score is the mean of lse over its frames (NaN for a row without frames); an utterance's
 * back-end score is mean lse_bona - mean lse_spoof.  An empty component ends at mu = 0, var = reg_covar.
 *
 * Frames: layout 0 is frame-major (B, Tcap, D) - (N, D) is B = 1 - and layout 1 the models' (B, D, Tcap).  n_frames is
 * int32 (B) on the device or NULL (every row full): row b contributes the frames t < min(max(n_frames[b], 0), Tcap).
 * Nothing else is read into the arithmetic: the other frames are replaced by zeros before they reach an MFMA and
 * carry r = 0, so NaN padding changes nothing.  1 <= K <= 1024, 1 <= D <= 128, B * Tcap < 2^31; anything else is
 * AIR_EUNSUPPORTED (layout outside {0, 1}, B or Tcap < 1: AIR_EINVAL) before any HIP call.
 *
 * air_gmm_prepare packs the model for the E-step into params (air_gmm_params_doubles(K, D) fp64): per tile of 16
 * components the MFMA B operand [feature j][component], j < Dp: mu p, Dp <= j < 2 Dp: -0.5 p (Dp = D padded to 8, 32,
 * 64 or 128, zeros in the padding), then the constants c_k (-inf for the padding components).
 * stats is air_gmm_stats_doubles(K, D) = K + 2 K D + 2 fp64: S0 (K), S1 (K, D), S2 (K, D), LL, and Nf as int64 in the
 * last 8 bytes.  air_gmm_accumulate ADDS this batch's sums to it (zero it to begin an iteration); calls accumulate in
 * stream order.  The (N, K) responsibilities never reach memory: pass A leaves lse per frame (8 bytes) and one (LL,
 * count) pair per tile of air_gmm_frame_tile() frames in ws; pass B recomputes the logits per (frame chunk x 64
 * components) workgroup and keeps its 64 x 2 Dp sums in registers; pass C adds the per-chunk partials in chunk order.
 * All products and sums are fp64 on v_mfma_f64_16x16x4_f64 where they are matrix products.  No atomics: the same call
 * on the same stats gives the same bits.  No host synchronisation in accumulate, loglik or mstep.
 * air_gmm_loglik: frame_ll (B * Tcap fp64, 0 for frames beyond a row's count) and / or row_ll (B fp64), either may be
 * NULL; ws as for accumulate (only the lse part is used when frame_ll is NULL).
 * air_gmm_mstep reads stats and writes w, mu, var and lower_bound (1 fp64) on the device.
 * air_gmm_ws_bytes(n_frames_cap = B * Tcap, K, D): 0 for sizes the calls refuse; a smaller ws: AIR_EWORKSPACE. */
int air_gmm_frame_tile(void);
size_t air_gmm_params_doubles(int K, int D);
size_t air_gmm_stats_doubles(int K, int D);
size_t air_gmm_ws_bytes(int64_t n_frames_cap, int K, int D);
int air_gmm_prepare(const double* w, const double* mu, const double* var, int K, int D, double* params,
                    air_stream_t stream);
int air_gmm_accumulate(const float* x, int layout, int B, int Tcap, const int* n_frames, const double* params, int K,
                       int D, double* stats, void* ws, size_t ws_bytes, air_stream_t stream);
int air_gmm_loglik(const float* x, int layout, int B, int Tcap, const int* n_frames, const double* params, int K, int D,
                   double* frame_ll, double* row_ll, void* ws, size_t ws_bytes, air_stream_t stream);
int air_gmm_mstep(const double* stats, int K, int D, double reg_covar, double* w, double* mu, double* var,
                  double* lower_bound, air_stream_t stream);
/* Measurement instrumentation, not part of the interface (like the air_debug_* entries above: it may change or go
 * without an ABI bump; only tools/bench_gmm.py calls it): nblocks workgroups of four waves, each wave `iters` rounds of four independent
 * v_mfma_f64_16x16x4_f64 (2048 flop each) with no memory traffic in the loop; out gets nblocks * 256 fp64.  The rate it
 * reaches is the measured fp64 matrix peak tools/bench_gmm.py holds the kernels against.  nblocks <= 65536,
 * iters <= 2^24. */
int air_debug_mfma_f64_probe(int nblocks, int iters, double* out, air_stream_t stream);

/* ------------------------------------------------------------ optimiser ---
 * torch.optim.Adam as configured at main_train.py:175-176 (coupled L2 weight
 * decay) and torch.optim.SGD(lr) (main_train.py:272), over flat fp32 buffers.
 * step is the 1-based step count.  grad_scale multiplies g first (1/world).
 */
int air_adam_step(float* p, const float* g, float* m, float* v, size_t n, int step, float lr,
                  float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                  air_stream_t stream);
int air_sgd_step(float* p, const float* g, size_t n, float lr, float grad_scale,
                 air_stream_t stream);

/* Test instrumentation: occupy `nblocks` compute units for `milliseconds` (<= 200) on `stream` - one 64-thread
 * workgroup per block holding `lds_bytes` of LDS and spinning on the wall clock.  Stands in for collective (RCCL)
 * kernels that are resident on some CUs while the persistent convolution kernels are dispatched
 * (tests/test_cu_mask_gpu.py); the reference has no counterpart (main_train.py:174 is a commented-out DataParallel). */
int air_debug_cu_hog(int nblocks, int lds_bytes, double milliseconds, air_stream_t stream);

/* Measurement instrumentation: one wave on `stream` that writes n_samples pairs {wall-clock ticks (100 MHz), core-clock
 * counter (s_memtime)} into out[2 * n_samples], one pair every interval_us (>= 1; n_samples * interval_us <= 5 s).
 * Launched on a side stream next to the training step it gives the clock the compute units run at under that kernel
 * mix (bench.py "core_clock"): the MFMA-dense kernels are power-capped below the 2.4 GHz the peak figures assume.
 * No reference counterpart. */
int air_debug_clock_probe(unsigned long long* out, int n_samples, double interval_us, air_stream_t stream);

/* ------------------------------------------------- bench instrumentation ---
 * Opt-in HIP-event timing of the dominant kernels on their launch stream, used
 * by bench.py's roofline leg only (off by default).  kid indexes the kernel
 * template instance (air_prof_kernel_name).  work = algorithmic FLOPs (conv) or
 * bytes (LFCC) summed over the recorded launches. */
int air_prof_enable(int on);
int air_prof_kernel_count(void);
const char* air_prof_kernel_name(int kid);
int air_prof_collect(int kid, int* launches, double* total_ms, double* total_work);
/* The same plus total_issued: the FLOPs those launches sent to the matrix pipe - equal to
 * total_work for the direct kernels, fewer for the Winograd kernels (36 or 30 multiplies per
 * 4x4 / 3x4 output tile, padded tiles included) - and total_bytes: their algorithmic HBM bytes
 * (every operand read once, every result written once; 0 for kernels that do not state it). */
int air_prof_collect2(int kid, int* launches, double* total_ms, double* total_work,
                      double* total_issued, double* total_bytes);

/* ------------------------------------------------------------- utility ---- */
int air_add_inplace(float* y, const float* x, size_t n, air_stream_t stream); /* y += x */

#ifdef __cplusplus
}
#endif
#endif /* AIR_HIP_H */
