// The decoded corpus in HBM (air_hip.h, "device corpus"): the random permutation of a flow, the ragged row copy that
// packs decoded batches into the flat store, and the gather that draws one training batch out of it.  Together they
// replace the two SubsetRandomSamplers, the collate functions and the crop draw of main_train.py:226-345 /
// dataset.py:69 without the host touching a sample.
//
// Random words: word(i, s) = word 0 of the Philox4x32-10 block at counter {i, s, 0, 0}, key {seed lo, seed hi} - the
// generator of air_philox.h / tests/philox_oracle.py.  s = (generation << 2) | kind: kind 0 / 1 the permutation of the
// first / second flow, kind 2 the crop offsets.
//
// Permutation of n: key_i = word(i, s) << 32 | i, padded with all-ones sentinels in the layout air_eval_sort_keys
// sorts (eval_metrics.hip: the first npad * 8 bytes of the workspace, npad the power of two >= max(n, sort block)),
// sorted by THAT sort; perm[j] = lo + (key_j & 0xffffffff).  The keys are distinct (i is part of them), so the order
// is the order of np.sort whatever the network does with equal keys.
//
// Copy: one workgroup per (tile of CP_TILE_BYTES, row).  Rows whose two ends are 16-byte aligned move 16 bytes per
// lane, the others single elements (a wave-uniform choice per row).  A chunk is copied whole only when it lies below
// the row's length; the chunk the length cuts is assembled element by element, so what lies behind a row in the
// store's alignment gap never reaches the output, and with a destination capacity [len, cap) is written as zeros.
#include <cstdint>

#include "air_common.h"
#include "air_philox.h"

namespace {

constexpr int CP_THREADS = 256;
constexpr int CP_TILE_BYTES = 8192;  // per workgroup: two 16-byte chunks per lane
constexpr int CP_KIND_CROP = 2;

__device__ __forceinline__ uint32_t cp_word(uint32_t i, uint32_t s, uint64_t seed) {
  uint32_t c[4];
  air_philox_block((uint64_t)s << 32 | i, seed, c);
  return c[0];
}

// keys[i], i < npad (a multiple of CP_THREADS)
__global__ __launch_bounds__(CP_THREADS) void cp_keys_kernel(uint64_t* __restrict__ keys, int n, uint64_t seed,
                                                             uint32_t s) {
  const int i = blockIdx.x * CP_THREADS + threadIdx.x;
  keys[i] = i < n ? ((uint64_t)cp_word((uint32_t)i, s, seed) << 32) | (uint32_t)i : ~0ull;
}

__global__ __launch_bounds__(CP_THREADS) void cp_perm_kernel(const uint64_t* __restrict__ keys, int n, long long lo,
                                                             long long* __restrict__ perm) {
  const int j = blockIdx.x * CP_THREADS + threadIdx.x;
  if (j < n) perm[j] = lo + (long long)(keys[j] & 0xffffffffull);
}

// Tile `tile` of one row: dst[e] = src[e] for e < len, 0 for len <= e < cap (cap 0: nothing is written past len).
// T is the element's bit pattern (uint16_t | uint32_t).  src is read at e < len only.
template <typename T>
__device__ __forceinline__ void cp_row_tile(const T* __restrict__ src, T* __restrict__ dst, int len, int cap, int tile) {
  constexpr int K = 16 / (int)sizeof(T);
  constexpr int TILE = CP_TILE_BYTES / (int)sizeof(T);
  const int begin = tile * TILE;
  const int end = min(begin + TILE, max(len, cap));
  if (begin >= end) return;
  if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {
    for (int e0 = begin + (int)threadIdx.x * K; e0 < end; e0 += CP_THREADS * K) {
      if (e0 + K <= len) {
        *reinterpret_cast<uint4*>(dst + e0) = *reinterpret_cast<const uint4*>(src + e0);
      } else if (e0 >= len && e0 + K <= cap) {
        *reinterpret_cast<uint4*>(dst + e0) = make_uint4(0u, 0u, 0u, 0u);
      } else {  // the chunk the length (or the capacity) cuts
        for (int e = e0; e < e0 + K; ++e) {
          if (e < len) dst[e] = src[e];
          else if (e < cap) dst[e] = (T)0;
        }
      }
    }
  } else {
    for (int e = begin + (int)threadIdx.x; e < end; e += CP_THREADS) dst[e] = e < len ? src[e] : (T)0;
  }
}

// row r: src + (src_off ? src_off[r] : r * src_stride), likewise dst; lengths clamped to [0, max_len]
template <typename T>
__global__ __launch_bounds__(CP_THREADS) void cp_copy_rows_kernel(const T* __restrict__ src,
                                                                  const long long* __restrict__ src_off,
                                                                  long long src_stride, T* __restrict__ dst,
                                                                  const long long* __restrict__ dst_off,
                                                                  long long dst_stride, const int* __restrict__ lengths,
                                                                  int max_len, int cap) {
  const int r = blockIdx.y;
  const int len = min(max(lengths[r], 0), max_len);
  const long long so = src_off ? src_off[r] : (long long)r * src_stride;
  const long long dof = dst_off ? dst_off[r] : (long long)r * dst_stride;
  cp_row_tile<T>(src + so, dst + dof, len, cap, blockIdx.x);
}

struct CpSeg {             // rows of one flow in a batch
  const long long* perm;   // its permutation, or nullptr: the identity
  long long first;         // first row of the permutation (identity: first corpus index)
  int count;
  uint32_t crop_stream;    // (generation << 2) | 2
};

struct CpGather {
  const void* store;
  const long long* offsets;   // element offset of every utterance
  const int* lengths;
  const long long* labels;
  const long long* tags;
  const long long* index;
  const long long* channels;  // (N, C) or nullptr
  long long N;
  int C, B, Lcap, feat_len, hop;
  uint64_t seed;
  CpSeg seg[2];
  void* pcm;
  int* out_lengths;
  long long* out_labels;
  long long* out_tags;
  long long* out_index;
  long long* out_channels;
  int* out_start;
};

template <typename T>
__global__ __launch_bounds__(CP_THREADS) void cp_gather_kernel(const CpGather g) {
  const int b = blockIdx.y;
  const int f = b < g.seg[0].count ? 0 : 1;
  const int r = f == 0 ? b : b - g.seg[0].count;
  const long long* perm = f == 0 ? g.seg[0].perm : g.seg[1].perm;
  const long long first = f == 0 ? g.seg[0].first : g.seg[1].first;
  const long long u = perm ? perm[first + r] : first + r;
  const bool ok = u >= 0 && u < g.N;  // (a row outside the corpus comes out empty instead of reading anywhere)
  const int full = ok ? max(g.lengths[u], 0) : 0;
  const int len = min(full, g.Lcap);
  const T* src = static_cast<const T*>(g.store) + (ok ? g.offsets[u] : 0);
  cp_row_tile<T>(src, static_cast<T*>(g.pcm) + (long long)b * g.Lcap, len, g.Lcap, blockIdx.x);
  if (blockIdx.x != 0) return;
  if (threadIdx.x == 0) {
    g.out_lengths[b] = len;
    g.out_labels[b] = ok ? g.labels[u] : 0;
    g.out_tags[b] = ok ? g.tags[u] : 0;
    g.out_index[b] = ok ? g.index[u] : -1;
    // dataset.py:69: np.random.randint(T - feat_len), T = 1 + len // hop frames; the exclusive bound stays
    const int frames = 1 + full / g.hop;
    int start = 0;
    if (frames > g.feat_len) {
      const uint32_t w = cp_word((uint32_t)u, f == 0 ? g.seg[0].crop_stream : g.seg[1].crop_stream, g.seed);
      start = (int)(((uint64_t)w * (uint64_t)(frames - g.feat_len)) >> 32);
    }
    g.out_start[b] = start;
  }
  if (g.channels != nullptr)
    for (int c = threadIdx.x; c < g.C; c += CP_THREADS) g.out_channels[(long long)b * g.C + c] = ok ? g.channels[u * g.C + c] : 0;
}

inline int cp_npad(int n) {
  int p = air_eval_sort_block();
  while (p < n) p <<= 1;
  return p;
}

inline int cp_tiles(int elems, int elem_bytes) {
  const int tile = CP_TILE_BYTES / elem_bytes;
  return (elems + tile - 1) / tile;
}

}  // namespace

extern "C" {

int air_corpus_copy_tile(int elem_bytes) { return (elem_bytes == 2 || elem_bytes == 4) ? CP_TILE_BYTES / elem_bytes : 0; }

size_t air_corpus_permutation_ws_bytes(int n) { return air_eval_workspace_bytes(n); }

int air_corpus_permutation(int64_t lo, int n, uint64_t seed, uint32_t stream_id, int64_t* perm_out, void* ws,
                           size_t ws_bytes, air_stream_t stream) {
  if (n < 1 || !perm_out || !ws || lo < 0) return AIR_EINVAL;
  if (n > air_eval_max_trials()) return AIR_EUNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(ws) & 15) != 0) return AIR_EINVAL;
  if (ws_bytes < air_eval_workspace_bytes(n)) return AIR_EWORKSPACE;
  hipStream_t st = air_stream(stream);
  uint64_t* keys = static_cast<uint64_t*>(ws);
  const int npad = cp_npad(n);  // a multiple of the sort block, itself a multiple of CP_THREADS
  cp_keys_kernel<<<npad / CP_THREADS, CP_THREADS, 0, st>>>(keys, n, seed, stream_id);
  AIR_CHECK_LAUNCH();
  const int rc = air_eval_sort_keys(n, ws, ws_bytes, stream);
  if (rc != AIR_OK) return rc;
  cp_perm_kernel<<<(n + CP_THREADS - 1) / CP_THREADS, CP_THREADS, 0, st>>>(keys, n, (long long)lo,
                                                                           reinterpret_cast<long long*>(perm_out));
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

int air_corpus_copy_rows(const void* src, const int64_t* src_off, int64_t src_stride, void* dst, const int64_t* dst_off,
                         int64_t dst_stride, const int* lengths, int rows, int max_len, int dst_cap, int elem_bytes,
                         air_stream_t stream) {
  if (!src || !dst || !lengths || rows < 0 || max_len < 0 || dst_cap < 0) return AIR_EINVAL;
  if (elem_bytes != 2 && elem_bytes != 4) return AIR_EUNSUPPORTED;
  if (rows > 65535) return AIR_EUNSUPPORTED;
  if (dst_cap > 0 && (dst_off != nullptr || dst_stride < dst_cap || max_len > dst_cap)) return AIR_EINVAL;
  if (!src_off && src_stride < max_len) return AIR_EINVAL;
  const int span = max_len > dst_cap ? max_len : dst_cap;
  if (rows == 0 || span == 0) return AIR_OK;
  const dim3 grid(cp_tiles(span, elem_bytes), rows);
  hipStream_t st = air_stream(stream);
  const long long* so = reinterpret_cast<const long long*>(src_off);
  const long long* dof = reinterpret_cast<const long long*>(dst_off);
  if (elem_bytes == 2)
    cp_copy_rows_kernel<uint16_t><<<grid, CP_THREADS, 0, st>>>(static_cast<const uint16_t*>(src), so, src_stride,
                                                               static_cast<uint16_t*>(dst), dof, dst_stride, lengths,
                                                               max_len, dst_cap);
  else
    cp_copy_rows_kernel<uint32_t><<<grid, CP_THREADS, 0, st>>>(static_cast<const uint32_t*>(src), so, src_stride,
                                                               static_cast<uint32_t*>(dst), dof, dst_stride, lengths,
                                                               max_len, dst_cap);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

int air_corpus_gather(const air_corpus_view* c, const air_corpus_segment* seg, int nseg, uint64_t seed, int feat_len,
                      int hop, int Lcap, void* pcm, int* lengths, int64_t* labels, int64_t* tags, int64_t* channels,
                      int64_t* index, int* start, air_stream_t stream) {
  if (!c || !seg || !c->samples || !c->offsets || !c->lengths || !c->labels || !c->tags || !c->index) return AIR_EINVAL;
  if (!pcm || !lengths || !labels || !tags || !index || !start) return AIR_EINVAL;
  if (nseg < 1 || nseg > 2 || c->n < 1 || c->n_channels < 0 || hop < 1 || feat_len < 1) return AIR_EINVAL;
  if ((c->channels != nullptr) != (channels != nullptr) || (c->channels != nullptr && c->n_channels < 1)) return AIR_EINVAL;
  if (c->elem_bytes != 2 && c->elem_bytes != 4) return AIR_EUNSUPPORTED;
  if (Lcap < 8 || (Lcap & 7) != 0) return AIR_EINVAL;
  if ((reinterpret_cast<uintptr_t>(pcm) & 15) != 0) return AIR_EINVAL;
  CpGather g;
  g.store = c->samples;
  g.offsets = reinterpret_cast<const long long*>(c->offsets);
  g.lengths = c->lengths;
  g.labels = reinterpret_cast<const long long*>(c->labels);
  g.tags = reinterpret_cast<const long long*>(c->tags);
  g.index = reinterpret_cast<const long long*>(c->index);
  g.channels = reinterpret_cast<const long long*>(c->channels);
  g.N = c->n;
  g.C = c->n_channels;
  g.Lcap = Lcap;
  g.feat_len = feat_len;
  g.hop = hop;
  g.seed = seed;
  long long B = 0;
  for (int k = 0; k < 2; ++k) {
    g.seg[k].perm = nullptr;
    g.seg[k].first = 0;
    g.seg[k].count = 0;
    g.seg[k].crop_stream = CP_KIND_CROP;
    if (k >= nseg) continue;
    if (seg[k].count < 0 || seg[k].first < 0) return AIR_EINVAL;
    if (seg[k].generation >= (1u << 30)) return AIR_EUNSUPPORTED;
    g.seg[k].perm = reinterpret_cast<const long long*>(seg[k].perm);
    g.seg[k].first = seg[k].first;
    g.seg[k].count = seg[k].count;
    g.seg[k].crop_stream = (seg[k].generation << 2) | CP_KIND_CROP;
    B += seg[k].count;
  }
  if (B < 1 || B > 65535) return B < 1 ? AIR_EINVAL : AIR_EUNSUPPORTED;
  g.B = (int)B;
  g.pcm = pcm;
  g.out_lengths = lengths;
  g.out_labels = reinterpret_cast<long long*>(labels);
  g.out_tags = reinterpret_cast<long long*>(tags);
  g.out_index = reinterpret_cast<long long*>(index);
  g.out_channels = reinterpret_cast<long long*>(channels);
  g.out_start = start;
  const dim3 grid(cp_tiles(Lcap, c->elem_bytes), (int)B);
  hipStream_t st = air_stream(stream);
  if (c->elem_bytes == 2)
    cp_gather_kernel<uint16_t><<<grid, CP_THREADS, 0, st>>>(g);
  else
    cp_gather_kernel<uint32_t><<<grid, CP_THREADS, 0, st>>>(g);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

}  // extern "C"
