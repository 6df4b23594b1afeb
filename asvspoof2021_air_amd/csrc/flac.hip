// FLAC decode of a batch of files into a ragged (B, Lcap) PCM batch (raw_dataset.py:20-28: librosa.load / sf.read of
// the corpus' 16 kHz, 16-bit, mono .flac files).  Served: the fixed-block-size subset of RFC 9639, mono, 16 bit - see
// include/air_hip.h.  Integer arithmetic throughout: the output is the encoder's input, bit for bit.
//
// A frame's length is not in its header, so frames are located before they are decoded:
//   flac_tail     zero samples [lengths[b], Lcap) of every row.
//   flac_scan     one thread per byte position: is a frame header consistent with the row here (sync, valid codes, mono,
//                 16 bit, block size <= the row's, CRC-8)?  One bit per position, a wave writes its 64 as one word.
//   flac_compact  one wave per row: the set bits of the row in position order -> candidate records in the row's slots.
//   flac_prefix   exclusive sum of the rows' candidate counts (the dense candidate index parse / decode iterate over).
//   flac_parse    one LANE per candidate: walk subframe and residual bitstream WITHOUT reconstructing samples; record
//                 the end offset, the CRC-16 verdict, block size, frame number.
//   flac_chain    one lane per row: from offset 0 follow end offsets from candidate to candidate; every frame needs a
//                 matching CRC-16 and the next frame number; the chain must end at the row's last byte with lengths[b]
//                 samples.  Chain frames are marked; the row's status says what failed first.
//   flac_decode   one LANE per marked frame of a row with status OK: Rice decode, predictor, wasted bits, store at
//                 frame_number * blocksize.
// A sync pattern inside a payload is a candidate and is parsed, but is never on the chain: it is never decoded.
//
// Lane per frame, not wave per frame: a frame is a serial bitstream (each Rice code starts where the last one ended)
// feeding a serial recurrence (each sample needs the 1 .. 32 before it); the parallelism is the ~14 frames x B rows of a
// batch.  Candidates are dealt to waves round-robin (candidate g -> wave g % waves, lane g / waves), so a batch smaller
// than the chip's wave slots runs one or two frames per wave: the lanes of a wave then do not gather from 64 frames
// at once, and the latency of the chain is one frame's.  The predictor history (32 samples) and the coefficients live
// in LDS, one column per lane ([k][lane]: a lane owns a bank, no conflicts).
//
// Bounds: every read of `bytes` is inside the row ([start, end) checked against total_bytes); the bit reader feeds
// zeros past the row's end and says so (over()); block sizes, partition counts, unary runs and escape widths are
// checked before they size a loop, and every loop over the stream ends when the reader is over.  Candidate slots: two
// candidates are >= 5 bytes apart (the bytes at +1 .. +4 of a valid header cannot start one), a row of n bytes has
// n / 4 slots; compaction checks the slot count all the same.
#include "air_common.h"

namespace {

constexpr int kScanThreads = 256;
constexpr int kLaneBlock = 64;       // parse / decode: one wave per workgroup
constexpr int kLaneWaves = 1024;     // waves the candidates are dealt over
constexpr uint32_t kMaxBlock = 65536;

// candidate record: 16 bytes
struct FlacRec {
  uint32_t pos;   // header offset in the row
  uint32_t end;   // one past the frame's CRC-16, in the row (parse)
  uint32_t fn;    // frame number
  uint32_t info;  // [16:0] samples, [24:20] header bytes, flags
};
constexpr uint32_t kRecSamples = 0x1ffffu;
constexpr uint32_t kRecCrcOk = 1u << 17;
constexpr uint32_t kRecInvalid = 1u << 18;
constexpr uint32_t kRecUnsupported = 1u << 19;
constexpr int kRecHdrShift = 20;
constexpr uint32_t kRecInChain = 1u << 25;

enum { WALK_OK = 0, WALK_INVALID = 1, WALK_UNSUPPORTED = 2 };

struct FlacWs {
  unsigned long long* mask;  // nwords
  FlacRec* rec;              // nslots
  int* ncand;                // B
  int* overflow;             // B
  int* cand_base;            // B + 1
  size_t nwords, nslots, bytes;
};

__host__ __device__ inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

inline FlacWs flac_ws_layout(void* ws, size_t total_bytes, int B) {
  FlacWs w;
  w.nwords = (total_bytes + 63) / 64;
  w.nslots = total_bytes / 4 + 1;
  char* p = (char*)ws;
  size_t o = 0;
  w.mask = (unsigned long long*)(p + o); o += up16(w.nwords * 8);
  w.rec = (FlacRec*)(p + o); o += up16(w.nslots * sizeof(FlacRec));
  w.ncand = (int*)(p + o); o += up16((size_t)B * 4);
  w.overflow = (int*)(p + o); o += up16((size_t)B * 4);
  w.cand_base = (int*)(p + o); o += up16(((size_t)B + 1) * 4);
  w.bytes = o;
  return w;
}

// row b = bytes [start, end): false (an empty row) when byte_off is not usable
__device__ __forceinline__ bool row_span(const int* __restrict__ byte_off, int b, uint32_t total, uint32_t& start, uint32_t& end) {
  const int o0 = byte_off[b], o1 = byte_off[b + 1];
  start = end = 0;
  if (o0 < 0 || o1 < 0) return false;
  const uint32_t s = ((uint32_t)o0 + 3u) & ~3u, e = (uint32_t)o1;
  if (s > e || e > total) return false;
  start = s;
  end = e;
  return true;
}

__device__ __forceinline__ uint32_t row_blocksize(const int* __restrict__ blocksize, int b) {
  const int v = blocksize[b];
  return v < 1 ? 0u : ((uint32_t)v > kMaxBlock ? kMaxBlock : (uint32_t)v);
}

// Frame header at p (avail bytes to the row's end).  0: not a frame; 1: a served frame header (CRC-8 matches, block
// size <= row_bs); 2: the sync code is there, with fields outside the served subset.
__host__ __device__ inline int flac_header(const uint8_t* __restrict__ p, uint32_t avail, uint32_t row_bs, uint32_t& bs, uint32_t& fn, uint32_t& hdr_bytes) {
  if (avail < 6) return 0;
  const uint32_t b0 = p[0], b1 = p[1];
  if (b0 != 0xFFu || (b1 & 0xFCu) != 0xF8u) return 0;
  const uint32_t b2 = p[2], b3 = p[3];
  const uint32_t bsc = b2 >> 4, src = b2 & 15u, ch = b3 >> 4, sz = (b3 >> 1) & 7u;
  if ((b1 & 3u) != 0 || bsc == 0 || src == 15u || (b3 & 1u) != 0 || ch != 0 || !(sz == 0 || sz == 4)) return 2;
  const uint32_t c0 = p[4];
  uint32_t extra, v;
  if (c0 < 0x80u) { extra = 0; v = c0; }
  else if ((c0 & 0xE0u) == 0xC0u) { extra = 1; v = c0 & 0x1Fu; }
  else if ((c0 & 0xF0u) == 0xE0u) { extra = 2; v = c0 & 0x0Fu; }
  else if ((c0 & 0xF8u) == 0xF0u) { extra = 3; v = c0 & 0x07u; }
  else if ((c0 & 0xFCu) == 0xF8u) { extra = 4; v = c0 & 0x03u; }
  else if ((c0 & 0xFEu) == 0xFCu) { extra = 5; v = c0 & 0x01u; }
  else return 0;
  const uint32_t nbs = bsc == 6 ? 1u : (bsc == 7 ? 2u : 0u);
  const uint32_t nsr = src == 12 ? 1u : ((src == 13 || src == 14) ? 2u : 0u);
  const uint32_t n = 5 + extra + nbs + nsr;  // bytes before the CRC-8: <= 14
  if (avail < n + 1) return 0;
  for (uint32_t i = 0; i < extra; ++i) {
    const uint32_t c = p[5 + i];
    if ((c & 0xC0u) != 0x80u) return 0;
    v = (v << 6) | (c & 0x3Fu);
  }
  uint32_t q = 5 + extra;
  if (bsc == 1) bs = 192;
  else if (bsc <= 5) bs = 576u << (bsc - 2);
  else if (bsc == 6) bs = (uint32_t)p[q] + 1;
  else if (bsc == 7) bs = (((uint32_t)p[q] << 8) | p[q + 1]) + 1;
  else bs = 256u << (bsc - 8);
  uint32_t crc = 0;
  for (uint32_t i = 0; i < n; ++i) {
    crc ^= p[i];
    for (int k = 0; k < 8; ++k) crc = (crc & 0x80u) ? ((crc << 1) ^ 0x07u) & 0xFFu : (crc << 1) & 0xFFu;
  }
  if (crc != p[n]) return 0;
  if (bs > row_bs) return 0;
  fn = v;
  hdr_bytes = n + 1;
  return 1;
}

// MSB-first bit reader over the `len` bytes at p.  Past the end it feeds zeros; over() says that more bits were
// consumed than the row holds.  No byte outside [p, p + len) is loaded.
struct BitReader {
  const uint8_t* __restrict__ p;
  uint32_t len, pos;  // pos: next byte to load (runs past len while zeros are fed)
  uint64_t buf;       // next bits at the top; the bits below the n valid ones are zero
  int n;

  __host__ __device__ __forceinline__ void seek(uint64_t bitpos) {
    const uint64_t lim = ((uint64_t)len << 3) + 64;
    if (bitpos > lim) bitpos = lim;  // over() holds from here on
    pos = (uint32_t)(bitpos >> 3);
    buf = 0;
    n = 0;
    refill();
    const int drop = (int)(bitpos & 7);
    buf <<= drop;
    n -= drop;
  }
  __host__ __device__ __forceinline__ void refill() {
    while (n <= 56) {
      const uint64_t b = pos < len ? (uint64_t)p[pos] : 0;
      buf |= b << (56 - n);
      n += 8;
      ++pos;
    }
  }
  __host__ __device__ __forceinline__ uint64_t bitpos() const { return ((uint64_t)pos << 3) - (uint64_t)n; }
  __host__ __device__ __forceinline__ bool over() const { return bitpos() > ((uint64_t)len << 3); }
  __host__ __device__ __forceinline__ uint32_t read(int nb) {  // 0 .. 32 bits
    if (nb == 0) return 0;
    refill();
    const uint32_t v = (uint32_t)(buf >> (64 - nb));
    buf <<= nb;
    n -= nb;
    return v;
  }
  __host__ __device__ __forceinline__ int32_t read_signed(int nb) {
    if (nb == 0) return 0;
    const uint32_t v = read(nb);
    return (int32_t)(v << (32 - nb)) >> (32 - nb);
  }
  // zero bits before the next one bit (consumed too).  Ends at the end of the row: over() then holds.
  __host__ __device__ __forceinline__ uint32_t unary() {
    uint32_t q = 0;
    for (;;) {
      refill();
      if (buf == 0) {
        q += (uint32_t)n;
        n = 0;
        if (pos > len) { refill(); return q; }  // only zeros are left: stop, over() after one more bit
        continue;
      }
      const int z = __builtin_clzll(buf);
      q += (uint32_t)z;
      buf = (buf << z) << 1;  // z + 1 can be 64
      n -= z + 1;
      return q;
    }
  }
  __host__ __device__ __forceinline__ void skip(uint64_t nbits) { seek(bitpos() + nbits); }
};

// Residual of one subframe: emit(i, r) for i = order .. bs - 1 (DEC), or only walked.
template <bool DEC, typename Emit>
__host__ __device__ __forceinline__ int flac_residual(BitReader& rd, uint32_t bs, uint32_t order, Emit&& emit) {
  const uint32_t method = rd.read(2);
  if (method > 1) return WALK_UNSUPPORTED;
  const uint32_t po = rd.read(4);
  const uint32_t psize = bs >> po;
  if ((psize << po) != bs || psize < order) return WALK_INVALID;
  const int pbits = method ? 5 : 4;
  const uint32_t esc = method ? 31u : 15u;
  uint32_t i = order;
  const uint32_t nparts = 1u << po;
  for (uint32_t part = 0; part < nparts; ++part) {
    const uint32_t cnt = part == 0 ? psize - order : psize;
    const uint32_t k = rd.read(pbits);
    if (k == esc) {
      const int nb = (int)rd.read(5);
      if (!DEC) {
        rd.skip((uint64_t)cnt * (uint32_t)nb);
      } else {
        for (uint32_t c = 0; c < cnt; ++c) emit(i++, rd.read_signed(nb));
      }
    } else {
      for (uint32_t c = 0; c < cnt; ++c) {
        const uint32_t q = rd.unary();
        const uint32_t u = (q << k) | rd.read((int)k);
        if (DEC) emit(i++, (int32_t)((u >> 1) ^ (0u - (u & 1u))));
        if (rd.over()) return WALK_INVALID;
      }
    }
    if (rd.over()) return WALK_INVALID;
  }
  return WALK_OK;
}

// One frame's subframe, from the bit behind the header (p = the frame's first byte, len = bytes to the row's end).
// DEC: store(i, sample) for i = 0 .. bs - 1; hist / coef: this lane's LDS columns (stride 64).  end_bytes: the frame's
// length up to and excluding the CRC-16.
template <bool DEC, typename Store>
__host__ __device__ int flac_frame(const uint8_t* __restrict__ p, uint32_t len, uint32_t hdr_bytes, uint32_t bs, int32_t* hist, int32_t* coef,
                          Store&& store, uint32_t& end_bytes) {
  BitReader rd;
  rd.p = p;
  rd.len = len;
  rd.seek((uint64_t)hdr_bytes << 3);
  if (rd.read(1)) return WALK_INVALID;
  const uint32_t type = rd.read(6);
  uint32_t wasted = 0;
  if (rd.read(1)) wasted = rd.unary() + 1;
  if (rd.over() || wasted >= 16) return WALK_INVALID;
  const int bps = 16 - (int)wasted;
  auto out = [&](uint32_t i, int32_t s) { store(i, (int32_t)((uint32_t)s << wasted)); };
  int rc = WALK_OK;
  if (type == 0) {  // CONSTANT
    const int32_t v = rd.read_signed(bps);
    if (DEC) for (uint32_t i = 0; i < bs; ++i) out(i, v);
  } else if (type == 1) {  // VERBATIM
    if (!DEC) {
      rd.skip((uint64_t)bs * (uint32_t)bps);
    } else {
      for (uint32_t i = 0; i < bs; ++i) out(i, rd.read_signed(bps));
    }
  } else if ((type >= 8 && type <= 12) || type >= 32) {  // FIXED 0..4 / LPC 1..32
    const bool lpc = type >= 32;
    const uint32_t order = lpc ? type - 31 : type - 8;
    if (order > bs) return WALK_INVALID;
    if (!DEC) {
      rd.skip((uint64_t)order * (uint32_t)bps);
    } else {
      for (uint32_t i = 0; i < order; ++i) {
        const int32_t s = rd.read_signed(bps);
        hist[(i & 31u) * 64] = s;
        out(i, s);
      }
    }
    int shift = 0;
    if (lpc) {
      const uint32_t prec = rd.read(4) + 1;
      if (prec == 16) return WALK_UNSUPPORTED;
      shift = rd.read_signed(5);
      if (shift < 0) return WALK_UNSUPPORTED;
      if (!DEC) {
        rd.skip((uint64_t)order * prec);
      } else {
        for (uint32_t j = 0; j < order; ++j) coef[j * 64] = rd.read_signed((int)prec);
      }
    } else if (DEC) {
      // the fixed predictors as coefficients: s[i] = sum c[j] s[i - 1 - j]
      const int32_t c1 = order == 1 ? 1 : (order == 2 ? 2 : (order == 3 ? 3 : 4));
      const int32_t c2 = order == 2 ? -1 : (order == 3 ? -3 : -6);
      const int32_t c3 = order == 3 ? 1 : 4;
      if (order >= 1) coef[0] = c1;
      if (order >= 2) coef[64] = c2;
      if (order >= 3) coef[128] = c3;
      if (order >= 4) coef[192] = -1;
    }
    if (rd.over()) return WALK_INVALID;
    rc = flac_residual<DEC>(rd, bs, order, [&](uint32_t i, int32_t r) {
      int64_t sum = 0;
      for (uint32_t j = 0; j < order; ++j) sum += (int64_t)coef[j * 64] * (int64_t)hist[((i - 1 - j) & 31u) * 64];
      const int32_t s = (int32_t)((uint32_t)r + (uint32_t)(int32_t)(sum >> shift));
      hist[(i & 31u) * 64] = s;
      out(i, s);
    });
  } else {
    return WALK_UNSUPPORTED;  // reserved subframe types
  }
  if (rc != WALK_OK) return rc;
  if (rd.over()) return WALK_INVALID;
  const uint64_t bits = rd.bitpos();
  const uint64_t bytes = (bits + 7) >> 3;  // zero padding to the byte boundary
  if (bytes + 2 > (uint64_t)len) return WALK_INVALID;
  end_bytes = (uint32_t)bytes;
  return WALK_OK;
}

// ------------------------------------------------------------------------------------------------ kernels
template <typename T>
__global__ __launch_bounds__(256) void flac_tail_kernel(T* __restrict__ y, const int* __restrict__ lengths, int Lcap) {
  const int b = blockIdx.y;
  int n = lengths[b];
  n = n < 0 ? 0 : (n > Lcap ? Lcap : n);
  T* row = y + (size_t)b * Lcap;
  for (int i = n + blockIdx.x * 256 + threadIdx.x; i < Lcap; i += gridDim.x * 256) row[i] = (T)0;
}

__global__ __launch_bounds__(kScanThreads) void flac_scan_kernel(const uint8_t* __restrict__ bytes, uint32_t total, const int* __restrict__ byte_off,
                                                                 const int* __restrict__ blocksize, int B,
                                                                 unsigned long long* __restrict__ mask, uint32_t nwords) {
  const uint32_t g = blockIdx.x * kScanThreads + threadIdx.x;
  bool cand = false;
  if (g + 1 < total && bytes[g] == 0xFFu && bytes[g + 1] == 0xF8u) {
    // the row of position g: the last b whose aligned start is <= g
    int lo = 0, hi = B - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      const int o = byte_off[mid];
      if (o >= 0 && (((uint32_t)o + 3u) & ~3u) <= g) lo = mid; else hi = mid - 1;
    }
    uint32_t start, end;
    if (row_span(byte_off, lo, total, start, end) && g >= start && g < end) {
      uint32_t bs, fn, hb;
      cand = flac_header(bytes + g, end - g, row_blocksize(blocksize, lo), bs, fn, hb) == 1;
    }
  }
  const unsigned long long m = __ballot(cand);
  if ((threadIdx.x & 63) == 0 && (g >> 6) < nwords) mask[g >> 6] = m;
}

__global__ __launch_bounds__(64) void flac_compact_kernel(const int* __restrict__ byte_off, uint32_t total, const unsigned long long* __restrict__ mask,
                                                          FlacRec* __restrict__ rec, int* __restrict__ ncand, int* __restrict__ overflow) {
  const int b = blockIdx.x, lane = threadIdx.x;
  uint32_t start, end;
  const bool ok = row_span(byte_off, b, total, start, end);
  uint32_t count = 0, cap = 0;
  bool ovf = false;
  if (ok && end > start) {
    cap = (end - start) >> 2;
    FlacRec* r = rec + (start >> 2);
    const uint32_t w0 = start >> 6, w1 = (end - 1) >> 6;
    for (uint32_t wb = w0; wb <= w1; wb += 64) {
      const uint32_t w = wb + lane;
      unsigned long long m = 0;
      if (w <= w1) {
        m = mask[w];
        const uint64_t first = (uint64_t)w << 6;
        if (first < start) m &= ~0ull << (start - first);
        if (first + 64 > end) m &= ~0ull >> (first + 64 - end);
      }
      const uint32_t c = (uint32_t)__popcll(m);
      uint32_t incl = c;
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
      }
      uint32_t idx = count + incl - c;
      while (m) {
        const int bit = __ffsll((long long)m) - 1;
        m &= m - 1;
        if (idx < cap) r[idx].pos = (uint32_t)(((uint64_t)w << 6) + bit - start); else ovf = true;
        ++idx;
      }
      count += __shfl(incl, 63, 64);
    }
  }
  ovf = __any(ovf);
  if (lane == 0) {
    ncand[b] = (int)(count < cap ? count : cap);
    overflow[b] = ovf ? 1 : 0;
  }
}

__global__ __launch_bounds__(256) void flac_prefix_kernel(const int* __restrict__ ncand, int B, int* __restrict__ cand_base) {
  __shared__ int part[256];
  const int t = threadIdx.x;
  const int per = (B + 255) / 256;
  const int lo = t * per < B ? t * per : B, hi = lo + per < B ? lo + per : B;
  int s = 0;
  for (int i = lo; i < hi; ++i) s += ncand[i];
  part[t] = s;
  __syncthreads();
  if (t == 0) {
    int acc = 0;
    for (int i = 0; i < 256; ++i) { const int v = part[i]; part[i] = acc; acc += v; }
    cand_base[B] = acc;
  }
  __syncthreads();
  int acc = part[t];
  for (int i = lo; i < hi; ++i) { cand_base[i] = acc; acc += ncand[i]; }
}

// candidate g of the dense index -> (row, record)
__device__ __forceinline__ int cand_row(const int* __restrict__ cand_base, int B, int g) {
  int lo = 0, hi = B - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (cand_base[mid] <= g) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(kLaneBlock) void flac_parse_kernel(const uint8_t* __restrict__ bytes, uint32_t total, const int* __restrict__ byte_off,
                                                                const int* __restrict__ blocksize, int B, FlacRec* __restrict__ rec,
                                                                const int* __restrict__ cand_base) {
  __shared__ uint16_t crc_tab[256];
  for (int i = threadIdx.x; i < 256; i += kLaneBlock) {
    uint32_t c = (uint32_t)i << 8;
    for (int k = 0; k < 8; ++k) c = (c & 0x8000u) ? ((c << 1) ^ 0x8005u) & 0xFFFFu : (c << 1) & 0xFFFFu;
    crc_tab[i] = (uint16_t)c;
  }
  __syncthreads();
  const int ntot = cand_base[B];
  const int nthreads = gridDim.x * kLaneBlock;
  for (int g = threadIdx.x * gridDim.x + blockIdx.x; g < ntot; g += nthreads) {
    const int b = cand_row(cand_base, B, g);
    uint32_t start, end;
    if (!row_span(byte_off, b, total, start, end)) continue;
    FlacRec* r = rec + (start >> 2) + (g - cand_base[b]);
    const uint32_t pos = r->pos;
    uint32_t info = kRecInvalid, fend = 0, fn = 0;
    if (pos < end - start) {
      const uint8_t* p = bytes + start + pos;
      const uint32_t len = end - start - pos;
      uint32_t bs = 0, hb = 0;
      if (flac_header(p, len, row_blocksize(blocksize, b), bs, fn, hb) == 1) {
        uint32_t eb = 0;
        const int rc = flac_frame<false>(p, len, hb, bs, nullptr, nullptr, [](uint32_t, int32_t) {}, eb);
        info = (bs & kRecSamples) | (hb << kRecHdrShift);
        if (rc == WALK_UNSUPPORTED) info |= kRecUnsupported;
        else if (rc != WALK_OK) info |= kRecInvalid;
        else {
          uint32_t crc = 0;
          for (uint32_t i = 0; i < eb; ++i) crc = ((crc << 8) & 0xFFFFu) ^ crc_tab[((crc >> 8) ^ p[i]) & 0xFFu];
          if (crc == (((uint32_t)p[eb] << 8) | p[eb + 1])) info |= kRecCrcOk;
          fend = pos + eb + 2;
        }
      }
    }
    r->end = fend;
    r->fn = fn;
    r->info = info;
  }
}

__global__ __launch_bounds__(64) void flac_chain_kernel(const uint8_t* __restrict__ bytes, uint32_t total, const int* __restrict__ byte_off,
                                                        const int* __restrict__ lengths, const int* __restrict__ blocksize, int B, int Lcap,
                                                        FlacRec* __restrict__ rec, const int* __restrict__ ncand,
                                                        const int* __restrict__ overflow, int* __restrict__ status) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  uint32_t start, end;
  int st = AIR_FLAC_OK;
  const int want = lengths[b];
  if (!row_span(byte_off, b, total, start, end)) st = AIR_FLAC_LOST_SYNC;
  else if (want < 0 || want > Lcap) st = AIR_FLAC_LENGTH_MISMATCH;
  else if (overflow[b]) st = AIR_FLAC_CANDIDATE_OVERFLOW;
  if (st == AIR_FLAC_OK) {
    const uint32_t len = end - start, row_bs = row_blocksize(blocksize, b);
    FlacRec* r = rec + (start >> 2);
    const int n = ncand[b];
    uint32_t expect = 0, fn = 0;
    int64_t samples = 0;
    bool short_seen = false;
    int idx = 0;
    while (expect < len) {
      while (idx < n && r[idx].pos < expect) ++idx;
      if (idx >= n || r[idx].pos != expect) {
        // no candidate here: a frame outside the served subset, or no frame at all
        uint32_t bs, f, hb;
        st = flac_header(bytes + start + expect, len - expect, row_bs, bs, f, hb) == 2 ? AIR_FLAC_UNSUPPORTED : AIR_FLAC_LOST_SYNC;
        break;
      }
      const uint32_t info = r[idx].info;
      if (info & kRecUnsupported) { st = AIR_FLAC_UNSUPPORTED; break; }
      if (info & kRecInvalid) { st = AIR_FLAC_LOST_SYNC; break; }
      if (!(info & kRecCrcOk)) { st = AIR_FLAC_BAD_CRC16; break; }
      if (r[idx].fn != fn) { st = AIR_FLAC_LOST_SYNC; break; }
      const uint32_t ns = info & kRecSamples;
      if (short_seen) { st = AIR_FLAC_LENGTH_MISMATCH; break; }  // only the last frame may be short
      if (ns != row_bs) short_seen = true;
      samples += ns;
      if (samples > want) { st = AIR_FLAC_LENGTH_MISMATCH; break; }
      const uint32_t e = r[idx].end;
      if (e <= expect || e > len) { st = AIR_FLAC_LOST_SYNC; break; }
      r[idx].info = info | kRecInChain;
      expect = e;
      ++fn;
      ++idx;
    }
    if (st == AIR_FLAC_OK && samples != want) st = AIR_FLAC_LENGTH_MISMATCH;
  }
  status[b] = st;
}

__global__ __launch_bounds__(kLaneBlock) void flac_decode_kernel(const uint8_t* __restrict__ bytes, uint32_t total, const int* __restrict__ byte_off,
                                                                 const int* __restrict__ lengths, const int* __restrict__ blocksize, int B, int Lcap,
                                                                 const FlacRec* __restrict__ rec, const int* __restrict__ cand_base,
                                                                 const int* __restrict__ status, int16_t* __restrict__ y16, float* __restrict__ y32) {
  __shared__ int32_t s_hist[32 * 64];
  __shared__ int32_t s_coef[32 * 64];
  int32_t* hist = s_hist + threadIdx.x;
  int32_t* coef = s_coef + threadIdx.x;
  const int ntot = cand_base[B];
  const int nthreads = gridDim.x * kLaneBlock;
  for (int g = threadIdx.x * gridDim.x + blockIdx.x; g < ntot; g += nthreads) {
    const int b = cand_row(cand_base, B, g);
    if (status[b] != AIR_FLAC_OK) continue;
    uint32_t start, end;
    if (!row_span(byte_off, b, total, start, end)) continue;
    const FlacRec r = rec[(start >> 2) + (g - cand_base[b])];
    if (!(r.info & kRecInChain)) continue;
    const uint32_t bs = r.info & kRecSamples, hb = (r.info >> kRecHdrShift) & 31u;
    if (r.pos >= end - start) continue;
    int lim = lengths[b];
    lim = lim < 0 ? 0 : (lim > Lcap ? Lcap : lim);
    const uint64_t off = (uint64_t)r.fn * row_blocksize(blocksize, b);
    if (off >= (uint64_t)lim) continue;
    const uint32_t room = (uint32_t)((uint64_t)lim - off);  // samples of this frame that are inside the row
    int16_t* o16 = y16 ? y16 + (size_t)b * Lcap + off : nullptr;
    float* o32 = y32 ? y32 + (size_t)b * Lcap + off : nullptr;
    uint32_t eb = 0;
    flac_frame<true>(bytes + start + r.pos, end - start - r.pos, hb, bs, hist, coef, [&](uint32_t i, int32_t s) {
      if (i < room) {
        const int16_t v = (int16_t)s;
        if (o16) o16[i] = v;
        if (o32) o32[i] = (float)v * (1.0f / 32768.0f);
      }
    }, eb);
  }
}

}  // namespace

extern "C" {

size_t air_flac_workspace_bytes(size_t total_bytes, int B) {
  if (B < 1 || total_bytes > (size_t)0x7fffffff) return 0;
  return flac_ws_layout(nullptr, total_bytes, B).bytes;
}

int air_flac_decode(const uint8_t* bytes, size_t total_bytes, const int* byte_off, const int* lengths, const int* blocksize,
                    int B, int Lcap, int16_t* y16, float* y32, int* status, void* ws, size_t ws_bytes, air_stream_t stream) {
  if (B < 1 || Lcap < 1 || total_bytes < 1 || total_bytes > (size_t)0x7fffffff) return AIR_EINVAL;
  if (!bytes || !byte_off || !lengths || !blocksize || !status || !ws || (!y16 && !y32)) return AIR_EINVAL;
  if (((uintptr_t)bytes & 3) || ((uintptr_t)ws & 15)) return AIR_EINVAL;
  if ((int64_t)B * Lcap > ((int64_t)1 << 40)) return AIR_EINVAL;
  const FlacWs w = flac_ws_layout(ws, total_bytes, B);
  if (ws_bytes < w.bytes) return AIR_EINVAL;
  hipStream_t st = air_stream(stream);
  const uint32_t total = (uint32_t)total_bytes;
  const dim3 tgrid((unsigned)((Lcap + 2047) / 2048 < 64 ? (Lcap + 2047) / 2048 : 64), (unsigned)B);
  if (B > 65535) return AIR_EUNSUPPORTED;
  if (y16) hipLaunchKernelGGL(flac_tail_kernel<int16_t>, tgrid, dim3(256), 0, st, y16, lengths, Lcap);
  if (y32) hipLaunchKernelGGL(flac_tail_kernel<float>, tgrid, dim3(256), 0, st, y32, lengths, Lcap);
  hipLaunchKernelGGL(flac_scan_kernel, dim3((unsigned)(w.nwords * 64 / kScanThreads + 1)), dim3(kScanThreads), 0, st, bytes, total, byte_off,
                     blocksize, B, w.mask, (uint32_t)w.nwords);
  hipLaunchKernelGGL(flac_compact_kernel, dim3((unsigned)B), dim3(64), 0, st, byte_off, total, w.mask, w.rec, w.ncand, w.overflow);
  hipLaunchKernelGGL(flac_prefix_kernel, dim3(1), dim3(256), 0, st, w.ncand, B, w.cand_base);
  hipLaunchKernelGGL(flac_parse_kernel, dim3(kLaneWaves), dim3(kLaneBlock), 0, st, bytes, total, byte_off, blocksize, B, w.rec, w.cand_base);
  hipLaunchKernelGGL(flac_chain_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, bytes, total, byte_off, lengths, blocksize, B, Lcap,
                     w.rec, w.ncand, w.overflow, status);
  hipLaunchKernelGGL(flac_decode_kernel, dim3(kLaneWaves), dim3(kLaneBlock), 0, st, bytes, total, byte_off, lengths, blocksize, B, Lcap, w.rec,
                     w.cand_base, status, y16, y32);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

}  // extern "C"
