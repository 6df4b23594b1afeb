// Exact DET-curve minima on the device: EER point and min t-DCF point of up to 2^20 trials, pooled and per group
// (air_hip.h, "evaluation metrics").  Replaces the sort + cumsum + argmin of eval_metrics.py:19-46 and the argmin over
// compute_tDCF's curve (eval_metrics.py:157-172, evaluate_tDCF_asvspoof19.py:58-59).
//
// One 64-bit key per trial: (order-preserving image of the fp32 score) << 9 | is_spoof << 8 | code.  The reference's
// stable mergesort of [bona fide..., spoof...] orders trials by score with bona fide first among equal scores; only the
// cumulative class counts at each curve point matter, and equal keys are interchangeable, so ANY correct sort of the
// keys gives the reference's curve.  -0.0 is canonicalised to +0.0 (numpy compares them equal), NaN is counted and
// refused by the caller.  Integers up to the two fp64 divisions per point, which are correctly rounded on both sides
// (the build has -ffp-contract=off): results are bit-equal to the host code or an error.
//
// code is the trial's group for the per-attack / per-channel breakdown: group + 1, 0 = "member of every group" (every
// trial of a call without groups), 255 = "of none" (an id out of range).  It rides below the class bit, so within equal
// scores bona fide still comes first inside every subset; any subset of a sorted sequence is sorted, so ONE sort serves
// the pooled curve and every group's: a record's curve is the walk over the same keys that counts its members only.
// Record 0 is the pooled one (every key a member), record 1 + g group g's.
//
// Sort: bitonic network over npad = max(EV_BLOCK, next power of two >= n) keys, padded with all-ones sentinels (above
// every real key: real keys stay below 2^41).  Sub-sequences of EV_BLOCK keys are sorted / merged in LDS, the strides
// >= EV_BLOCK run in global memory, one launch per stride.  EV_BLOCK * 8 B = 32 KiB per workgroup: five workgroups fit
// the 160 KiB of a CU, the 8 waves of each keep four resident under the 32-wave cap.
//
// Behind the sort: ev_counts_kernel takes the class / NaN / inf counts per sort block and record (a histogram of the
// codes for the groups), ev_prefix_kernel the exclusive prefix over the blocks per record and the record's totals,
// ev_curve_kernel walks each block once per record (blocks without a member of the record are skipped),
// ev_final_kernel reduces the blocks' candidates.  ev_prefix_kernel and ev_final_kernel write every word of a record
// between them and nothing writes one before ev_prefix_kernel: no memset.
#include "air_common.h"

#define EV_BLOCK 4096
#define EV_THREADS 512
#define EV_PER_THREAD (EV_BLOCK / EV_THREADS)
#define EV_MAX_N (1 << 20)
#define EV_MAX_BLOCKS (EV_MAX_N / EV_BLOCK)
#define EV_MAX_GROUPS 128
#define EV_CODE_BITS 8                    // group code below the class bit: 0 every group, 1 + g, 255 none
#define EV_CODE_MASK 255u
#define EV_CODE_NONE 255u
#define EV_IMG_SHIFT (EV_CODE_BITS + 1)   // the score's image sits above code and class bit
#define EV_CURVE_WGS 2048                 // workgroups the walk aims at: records are dealt over gridDim.y

static_assert(EV_MAX_GROUPS + 1 < (int)EV_CODE_NONE, "the codes 1 .. EV_MAX_GROUPS stay below the 'no group' code");
static_assert(EV_MAX_BLOCKS <= 256, "ev_prefix_kernel / ev_final_kernel take one block of the sort per thread");
static_assert(EV_BLOCK < (1 << 16), "ev_counts_kernel / ev_curve_kernel pack two per-block counts into 32 bits");

static_assert(sizeof(air_eval_record) == 64, "air_eval_record is 64 bytes");

namespace {

struct EvBest {  // 24 bytes: one candidate of the lexicographic (value, index) minimum on a record's own curve
  double v;
  uint32_t k;   // curve point: the k lowest members rejected
  uint32_t rn;  // spoof members among them
  uint32_t at;  // sorted position of the k-th member + 1 (0 at k = 0)
  uint32_t pad;
};

// b = the better of b and c, field by field (a whole-struct copy out of LDS leaves k, rn, at in a private array)
__device__ __forceinline__ void ev_take_better(EvBest& b, const EvBest& c) {
  if (c.v < b.v || (c.v == b.v && c.k < b.k)) {
    b.v = c.v;
    b.k = c.k;
    b.rn = c.rn;
    b.at = c.at;
  }
}

__device__ __forceinline__ EvBest ev_wave_best(EvBest b) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    EvBest c;
    c.v = __shfl_xor(b.v, o, 64);
    c.k = __shfl_xor(b.k, o, 64);
    c.rn = __shfl_xor(b.rn, o, 64);
    c.at = __shfl_xor(b.at, o, 64);
    c.pad = 0;
    ev_take_better(b, c);
  }
  return b;
}

__device__ __forceinline__ EvBest ev_none() {
  EvBest b;
  b.v = __longlong_as_double(0x7ff0000000000000ll);
  b.k = 0xffffffffu;
  b.rn = b.at = b.pad = 0;
  return b;
}

__device__ __forceinline__ uint32_t ev_wave_sum_u(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ uint32_t ev_image_bits(uint32_t o) {  // the fp32 bit pattern behind a key's score image
  return (o & 0x80000000u) ? (o ^ 0x80000000u) : ~o;
}

// keys[i] for i < npad (a multiple of the 1024 keys of a workgroup).  groups == nullptr: code 0 for every trial;
// else ids outside -1 .. n_groups - 1 get the code "of none"
template <typename L, typename Gt>
__global__ __launch_bounds__(256) void ev_keys_kernel(const float* __restrict__ scores, const L* __restrict__ labels,
                                                       const Gt* __restrict__ groups, int n, int npad, int negate,
                                                       int n_groups, uint64_t* __restrict__ keys) {
  const int base = blockIdx.x * (256 * 4);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int i = base + e * 256 + threadIdx.x;
    uint64_t key = ~0ull;
    if (i < n) {
      uint32_t u = __float_as_uint(scores[i]);
      if (negate) u ^= 0x80000000u;
      if ((u & 0x7fffffffu) == 0u) u = 0u;  // -0.0 -> +0.0
      const uint32_t spoof = labels[i] != 0;
      uint32_t code = 0u;
      if (groups != nullptr) {
        const long long g = (long long)groups[i];
        code = (g >= -1 && g < (long long)n_groups) ? (uint32_t)(g + 1) : EV_CODE_NONE;
      }
      const uint32_t o = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
      key = ((uint64_t)o << EV_IMG_SHIFT) | ((uint64_t)spoof << EV_CODE_BITS) | code;
    }
    keys[i] = key;
  }
}

__device__ __forceinline__ void ev_cmpx(uint64_t* s, int i, int j, bool asc) {
  const uint64_t a = s[i], b = s[i | j];
  if ((a > b) == asc) {
    s[i] = b;
    s[i | j] = a;
  }
}

// the steps j < EV_BLOCK of the stages k = kfirst .. klast of the network, on the EV_BLOCK keys of this workgroup:
// sort (kfirst = 2, klast = EV_BLOCK, every stage from its own j = k / 2) or the tail of one global stage
// (kfirst = klast = k > EV_BLOCK, j from EV_BLOCK / 2)
__global__ __launch_bounds__(EV_THREADS) void ev_sort_block_kernel(uint64_t* __restrict__ keys, int kfirst, int klast) {
  __shared__ uint64_t s[EV_BLOCK];
  const size_t base = (size_t)blockIdx.x * EV_BLOCK;
  for (int i = threadIdx.x; i < EV_BLOCK; i += EV_THREADS) s[i] = keys[base + i];
  __syncthreads();
  for (int k = kfirst; k <= klast; k <<= 1) {
    const int j0 = k > EV_BLOCK ? EV_BLOCK / 2 : k / 2;
    for (int j = j0; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < EV_BLOCK / 2; t += EV_THREADS) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        ev_cmpx(s, i, j, ((base + i) & (size_t)k) == 0);
      }
      __syncthreads();
    }
  }
  for (int i = threadIdx.x; i < EV_BLOCK; i += EV_THREADS) keys[base + i] = s[i];
}

// one step (stride j >= EV_BLOCK) of stage k over npad keys, one pair per thread
__global__ __launch_bounds__(256) void ev_merge_global_kernel(uint64_t* __restrict__ keys, int npad, int j, int k) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= npad / 2) return;
  const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
  const uint64_t a = keys[i], b = keys[i | j];
  if ((a > b) == ((i & k) == 0)) {
    keys[i] = b;
    keys[i | j] = a;
  }
}

// per EV_BLOCK of the sorted keys and per record r: blk[r][block] = {spoof members, bona fide members, sorted position
// + 1 of the block's last member (0: none), inf | NaN << 16 members}; none[block] = keys of no group.  Record 0 is
// every key: the block's sums.  With groups, one LDS histogram over the codes (integer atomics: sums and a maximum,
// independent of their order); record r >= 1 is code r plus code 0.
__global__ __launch_bounds__(256) void ev_counts_kernel(const uint64_t* __restrict__ keys, int n, int n_groups,
                                                         uint4* __restrict__ blk, uint32_t* __restrict__ none) {
  __shared__ uint32_t h_cls[256], h_last[256], h_bad[256];  // per code: spoof | bona fide << 16, last, inf | NaN << 16
  __shared__ uint32_t part[4][2];
  const int tid = threadIdx.x;
  h_cls[tid] = h_last[tid] = h_bad[tid] = 0;
  __syncthreads();
  const int base = blockIdx.x * EV_BLOCK;
  uint64_t mine[EV_BLOCK / 256];  // (all loads in flight before the first atomic)
#pragma unroll
  for (int e = 0; e < EV_BLOCK / 256; ++e) mine[e] = base + e * 256 + tid < n ? keys[base + e * 256 + tid] : ~0ull;
  uint32_t cls = 0, bad = 0;
#pragma unroll
  for (int e = 0; e < EV_BLOCK / 256; ++e) {
    const int i = e * 256 + tid;
    if (base + i < n) {
      const uint64_t key = mine[e];
      const uint32_t code = (uint32_t)key & EV_CODE_MASK;
      const uint32_t mag = ev_image_bits((uint32_t)(key >> EV_IMG_SHIFT)) & 0x7fffffffu;
      const uint32_t c = ((key >> EV_CODE_BITS) & 1ull) ? 1u : 0x10000u;
      const uint32_t b = (mag == 0x7f800000u ? 1u : 0u) | (mag > 0x7f800000u ? 0x10000u : 0u);
      cls += c;
      bad += b;
      if (n_groups) {  // (uniform; without groups every code is 0 and record 0 does not read the histogram)
        atomicAdd(&h_cls[code], c);
        atomicMax(&h_last[code], (uint32_t)(base + i) + 1u);
        if (b) atomicAdd(&h_bad[code], b);
      }
    }
  }
  cls = ev_wave_sum_u(cls);
  bad = ev_wave_sum_u(bad);
  if ((tid & 63) == 0) {
    part[tid >> 6][0] = cls;
    part[tid >> 6][1] = bad;
  }
  __syncthreads();
  if (tid <= n_groups) {
    uint32_t c, b, last;
    if (tid == 0) {
      c = part[0][0] + part[1][0] + part[2][0] + part[3][0];
      b = part[0][1] + part[1][1] + part[2][1] + part[3][1];
      last = (uint32_t)(n < base + EV_BLOCK ? n : base + EV_BLOCK);
      none[blockIdx.x] = (h_cls[EV_CODE_NONE] & 0xffffu) + (h_cls[EV_CODE_NONE] >> 16);
    } else {
      c = h_cls[tid] + h_cls[0];
      b = h_bad[tid] + h_bad[0];
      last = h_last[tid] > h_last[0] ? h_last[tid] : h_last[0];
    }
    blk[(size_t)tid * EV_MAX_BLOCKS + blockIdx.x] = make_uint4(c & 0xffffu, c >> 16, last, b);
  }
}

// per record (blockIdx.x): exclusive prefix of blk over the blocks (thread t = block t, fixed order) into
// pre[r][block] = {spoof members below the block, bona fide members below it, last member below it + 1, members in it}.
// The totals are the record's n_tar / n_non / n_nan / n_inf; this kernel is the first to write the record and leaves
// every field that ev_final_kernel does not write: n_distinct 0 (ev_curve_kernel counts into it), both *_score_first
// 0.0 (ev_curve_kernel, where the record has a member), reserved[0] the keys of no group in record 0.
__global__ __launch_bounds__(256) void ev_prefix_kernel(const uint4* __restrict__ blk, const uint32_t* __restrict__ none,
                                                         int nblk, uint4* __restrict__ pre, air_eval_record* recs) {
  __shared__ uint32_t tot[4][6];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = blockIdx.x;
  const uint4 v = tid < nblk ? blk[(size_t)r * EV_MAX_BLOCKS + tid] : make_uint4(0, 0, 0, 0);
  uint32_t non = v.x, tar = v.y, last = v.z, inf = v.w & 0xffffu, nan = v.w >> 16;
  uint32_t out = (r == 0 && tid < nblk) ? none[tid] : 0u;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t a = __shfl_up(non, o, 64), b = __shfl_up(tar, o, 64), c = __shfl_up(last, o, 64);
    if (lane >= o) {
      non += a;
      tar += b;
      last = c > last ? c : last;
    }
  }
  inf = ev_wave_sum_u(inf);
  nan = ev_wave_sum_u(nan);
  out = ev_wave_sum_u(out);
  uint32_t last_x = __shfl_up(last, 1, 64);  // exclusive
  if (lane == 0) last_x = 0;
  if (lane == 63) {
    tot[wave][0] = non;
    tot[wave][1] = tar;
    tot[wave][2] = last;
    tot[wave][3] = inf;
    tot[wave][4] = nan;
    tot[wave][5] = out;
  }
  __syncthreads();
  uint32_t non_x = non - v.x, tar_x = tar - v.y;
  for (int w = 0; w < wave; ++w) {
    non_x += tot[w][0];
    tar_x += tot[w][1];
    last_x = tot[w][2] > last_x ? tot[w][2] : last_x;
  }
  if (tid < nblk) pre[(size_t)r * EV_MAX_BLOCKS + tid] = make_uint4(non_x, tar_x, last_x, v.x + v.y);
  if (tid == 0) {
    recs[r].n_non = tot[0][0] + tot[1][0] + tot[2][0] + tot[3][0];
    recs[r].n_tar = tot[0][1] + tot[1][1] + tot[2][1] + tot[3][1];
    recs[r].n_inf = tot[0][3] + tot[1][3] + tot[2][3] + tot[3][3];
    recs[r].n_nan = tot[0][4] + tot[1][4] + tot[2][4] + tot[3][4];
    recs[r].n_distinct = 0;
    recs[r].eer_score_first = 0.0f;
    recs[r].dcf_score_first = 0.0f;
    recs[r].reserved[0] = tot[0][5] + tot[1][5] + tot[2][5] + tot[3][5];
    recs[r].reserved[1] = 0;
  }
}

// the walk: blockIdx.x = EV_BLOCK of the sorted keys (held in registers across the records), records blockIdx.y,
// blockIdx.y + gridDim.y, ...  Per record the inclusive scan of "member and spoof" / "member and bona fide", both error
// rates in fp64 from the record's own counts, the block's first minimum of |frr - far| and of the normalised t-DCF.
// Curve point k >= 1 of a record exists where sorted trial i is its k-th member; point 0 goes with the thread of sorted
// trial 0.  A member adds a distinct score when the member before it (in this thread, else the scanned "last member so
// far", else the prefix over the blocks) has another image.  c12 == nullptr: the weights c1s, c2s for every record.
__global__ __launch_bounds__(EV_THREADS) void ev_curve_kernel(const uint64_t* __restrict__ keys, int n, int n_groups,
                                                               const uint4* __restrict__ pre, int want_dcf,
                                                               const double* __restrict__ c12, double c1s, double c2s,
                                                               air_eval_record* recs, EvBest* __restrict__ partial) {
  __shared__ uint32_t wave_tot[EV_THREADS / 64], wave_last[EV_THREADS / 64];
  __shared__ EvBest best_s[2][EV_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int first = blockIdx.x * EV_BLOCK + tid * EV_PER_THREAD;
  uint64_t key[EV_PER_THREAD];
#pragma unroll
  for (int e = 0; e < EV_PER_THREAD; ++e) key[e] = first + e < n ? keys[first + e] : ~0ull;

  for (int r = blockIdx.y; r <= n_groups; r += gridDim.y) {
    const uint4 bs = pre[(size_t)r * EV_MAX_BLOCKS + blockIdx.x];
    EvBest* out = partial + ((size_t)r * EV_MAX_BLOCKS + blockIdx.x) * 2;
    if (bs.w == 0u && blockIdx.x != 0) {  // no member in this block (the whole workgroup takes this branch)
      if (tid < 2) out[tid] = ev_none();
      continue;
    }
    uint32_t member = 0, mine = 0, lastl = 0;  // spoof | bona fide << 16 members of this thread, its last member + 1
#pragma unroll
    for (int e = 0; e < EV_PER_THREAD; ++e) {
      const uint32_t code = (uint32_t)key[e] & EV_CODE_MASK;
      if (first + e < n && (r == 0 || code == 0u || code == (uint32_t)r)) {
        member |= 1u << e;
        mine += ((key[e] >> EV_CODE_BITS) & 1ull) ? 1u : 0x10000u;
        lastl = (uint32_t)(first + e) + 1u;
      }
    }
    uint32_t incl = mine, incl_last = lastl;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t up = __shfl_up(incl, o, 64), upl = __shfl_up(incl_last, o, 64);
      if (lane >= o) {
        incl += up;
        incl_last = upl > incl_last ? upl : incl_last;
      }
    }
    uint32_t prev = __shfl_up(incl_last, 1, 64);
    if (lane == 0) prev = 0;
    if (lane == 63) {
      wave_tot[wave] = incl;
      wave_last[wave] = incl_last;
    }
    __syncthreads();
    uint32_t excl = incl - mine;
    for (int w = 0; w < wave; ++w) {
      excl += wave_tot[w];
      prev = wave_last[w] > prev ? wave_last[w] : prev;
    }
    prev = bs.z > prev ? bs.z : prev;
    uint32_t rn = bs.x + (excl & 0xffffu), rt = bs.y + (excl >> 16);
    const uint32_t n_tar_u = recs[r].n_tar, n_non_u = recs[r].n_non;  // (in flight together with the key below)
    // (an image has 32 bits: no member before this one is the value no image takes)
    uint64_t pimg = (member != 0u && prev != 0u) ? (keys[prev - 1u] >> EV_IMG_SHIFT) : ~0ull;

    const double n_tar = (double)n_tar_u, n_non = (double)n_non_u;
    const double c1 = c12 != nullptr ? c12[2 * r] : c1s, c2 = c12 != nullptr ? c12[2 * r + 1] : c2s;
    const double cmin = c1 < c2 ? c1 : c2;
    EvBest eer = ev_none(), dcf = ev_none();
    uint32_t distinct = 0;
    if (first == 0) {  // curve point 0: nothing rejected, FRR 0, FAR 1
      const double frr = 0.0 / n_tar, far = (double)n_non_u / n_non;
      eer.v = fabs(frr - far);
      dcf.v = (c1 * frr + c2 * far) / cmin;
      eer.k = dcf.k = 0;
    }
#pragma unroll
    for (int e = 0; e < EV_PER_THREAD; ++e) {
      if (member & (1u << e)) {
        const uint32_t sp = (uint32_t)(key[e] >> EV_CODE_BITS) & 1u;
        rn += sp;
        rt += sp ^ 1u;
        const uint32_t k = rn + rt, at = (uint32_t)(first + e) + 1u;
        const uint64_t img = key[e] >> EV_IMG_SHIFT;
        distinct += img != pimg;
        pimg = img;
        if (k == 1u) {  // the record's lowest score (one thread per record)
          const float s0 = __uint_as_float(ev_image_bits((uint32_t)img));
          recs[r].eer_score_first = s0;
          recs[r].dcf_score_first = s0;
        }
        const double frr = (double)rt / n_tar;
        const double far = (double)(n_non_u - rn) / n_non;
        const double d = fabs(frr - far);
        if (d < eer.v) {
          eer.v = d;
          eer.k = k;
          eer.rn = rn;
          eer.at = at;
        }
        if (want_dcf) {
          const double t = (c1 * frr + c2 * far) / cmin;
          if (t < dcf.v) {
            dcf.v = t;
            dcf.k = k;
            dcf.rn = rn;
            dcf.at = at;
          }
        }
      }
    }
    eer = ev_wave_best(eer);
    dcf = ev_wave_best(dcf);
    distinct = ev_wave_sum_u(distinct);
    if (lane == 0) {
      best_s[0][wave] = eer;
      best_s[1][wave] = dcf;
      if (distinct) atomicAdd(&recs[r].n_distinct, distinct);
    }
    __syncthreads();
    if (tid < 2) {
      EvBest b = best_s[tid][0];
      for (int w = 1; w < EV_THREADS / 64; ++w) ev_take_better(b, best_s[tid][w]);
      out[tid] = b;
    }
    // (the next record writes wave_tot / wave_last behind this barrier and best_s behind its own first one)
  }
}

// per record (blockIdx.x): the first minimum over the blocks' candidates; the record's indices and scores
__global__ __launch_bounds__(256) void ev_final_kernel(const EvBest* __restrict__ partial, int nblk,
                                                        const uint64_t* __restrict__ keys, int want_dcf,
                                                        air_eval_record* recs) {
  __shared__ EvBest best_s[2][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  air_eval_record* rec = recs + blockIdx.x;
  EvBest b[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    b[q] = tid < nblk ? partial[((size_t)blockIdx.x * EV_MAX_BLOCKS + tid) * 2 + q] : ev_none();
    b[q] = ev_wave_best(b[q]);
    if (lane == 0) best_s[q][wave] = b[q];
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      EvBest m = best_s[q][0];
      for (int w = 1; w < 4; ++w) ev_take_better(m, best_s[q][w]);
      b[q] = m;
    }
    // (an empty class makes every value NaN and leaves the index at its initial value: the record then says so
    // through n_tar / n_non, and no key is read out of range)
    const float s0 = rec->eer_score_first;  // (ev_curve_kernel; 0.0 for a record without members)
    const uint32_t n = rec->n_tar + rec->n_non;
    rec->eer_idx = b[0].k;
    rec->eer_rej_non = b[0].rn;
    rec->eer_score_at = (b[0].k >= 1u && b[0].k <= n) ? __uint_as_float(ev_image_bits((uint32_t)(keys[b[0].at - 1u] >> EV_IMG_SHIFT))) : s0;
    rec->has_dcf = want_dcf ? 1u : 0u;
    rec->dcf_idx = want_dcf ? b[1].k : 0u;
    rec->dcf_rej_non = want_dcf ? b[1].rn : 0u;
    rec->dcf_score_at = (want_dcf && b[1].k >= 1u && b[1].k <= n) ? __uint_as_float(ev_image_bits((uint32_t)(keys[b[1].at - 1u] >> EV_IMG_SHIFT))) : s0;
  }
}

inline int ev_npad(int n) {
  int p = EV_BLOCK;
  while (p < n) p <<= 1;
  return p;
}

// workspace: keys[npad] | blk[G + 1][EV_MAX_BLOCKS] | pre[G + 1][EV_MAX_BLOCKS] | partial[G + 1][EV_MAX_BLOCKS][2] |
// none[EV_MAX_BLOCKS]
inline size_t ev_bytes(int n, int n_groups) {
  return (size_t)ev_npad(n) * 8 + (size_t)(n_groups + 1) * EV_MAX_BLOCKS * (2 * sizeof(uint4) + 2 * sizeof(EvBest)) +
         (size_t)EV_MAX_BLOCKS * 4;
}

inline int ev_check(int n, int n_groups, const void* ws, size_t ws_bytes) {
  if (n < 1 || ws == nullptr) return AIR_EINVAL;
  if (n > EV_MAX_N || n_groups < 0 || n_groups > EV_MAX_GROUPS) return AIR_EUNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(ws) & 15) != 0) return AIR_EINVAL;
  if (ws_bytes < ev_bytes(n, n_groups)) return AIR_EWORKSPACE;
  return AIR_OK;
}

template <typename L>
int ev_keys_launch(const float* scores, const L* labels, const void* groups, int group_bytes, int n, int negate,
                   int n_groups, uint64_t* keys, hipStream_t st) {
  const int npad = ev_npad(n);
  if (group_bytes == 8)
    ev_keys_kernel<L, int64_t><<<npad / 1024, 256, 0, st>>>(scores, labels, static_cast<const int64_t*>(groups), n, npad, negate,
                                                            n_groups, keys);
  else
    ev_keys_kernel<L, int32_t><<<npad / 1024, 256, 0, st>>>(scores, labels, static_cast<const int32_t*>(groups), n, npad, negate,
                                                            n_groups, keys);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

// the three steps of the chain on a checked workspace; n_groups == 0 (groups nullptr): the pooled record alone
int ev_keys(const float* scores, const void* labels, int label_bytes, const void* groups, int group_bytes, int n,
            int n_groups, int negate, void* ws, hipStream_t st) {
  uint64_t* keys = static_cast<uint64_t*>(ws);
  return label_bytes == 8 ? ev_keys_launch(scores, static_cast<const int64_t*>(labels), groups, group_bytes, n, negate ? 1 : 0,
                                           n_groups, keys, st)
                          : ev_keys_launch(scores, static_cast<const int32_t*>(labels), groups, group_bytes, n, negate ? 1 : 0,
                                           n_groups, keys, st);
}

int ev_sort(void* ws, int n, hipStream_t st) {
  uint64_t* keys = static_cast<uint64_t*>(ws);
  const int npad = ev_npad(n), nblk = npad / EV_BLOCK;
  ev_sort_block_kernel<<<nblk, EV_THREADS, 0, st>>>(keys, 2, EV_BLOCK);
  AIR_CHECK_LAUNCH();
  for (int k = 2 * EV_BLOCK; k <= npad; k <<= 1) {
    for (int j = k / 2; j >= EV_BLOCK; j >>= 1) {
      ev_merge_global_kernel<<<npad / 2 / 256, 256, 0, st>>>(keys, npad, j, k);
      AIR_CHECK_LAUNCH();
    }
    ev_sort_block_kernel<<<nblk, EV_THREADS, 0, st>>>(keys, k, k);
    AIR_CHECK_LAUNCH();
  }
  return AIR_OK;
}

int ev_curve_min(int n, int n_groups, int want_dcf, const double* c12, double c1, double c2, air_eval_record* recs,
                 void* ws, hipStream_t st) {
  const int nrec = n_groups + 1;
  char* p = static_cast<char*>(ws);
  const uint64_t* keys = reinterpret_cast<const uint64_t*>(p);
  p += (size_t)ev_npad(n) * 8;
  uint4* blk = reinterpret_cast<uint4*>(p);
  p += (size_t)nrec * EV_MAX_BLOCKS * sizeof(uint4);
  uint4* pre = reinterpret_cast<uint4*>(p);
  p += (size_t)nrec * EV_MAX_BLOCKS * sizeof(uint4);
  EvBest* partial = reinterpret_cast<EvBest*>(p);
  p += (size_t)nrec * EV_MAX_BLOCKS * 2 * sizeof(EvBest);
  uint32_t* none = reinterpret_cast<uint32_t*>(p);
  const int nblk = (n + EV_BLOCK - 1) / EV_BLOCK;  // curve point k >= 1 goes with sorted trial k - 1, point 0 with trial 0
  ev_counts_kernel<<<nblk, 256, 0, st>>>(keys, n, n_groups, blk, none);
  AIR_CHECK_LAUNCH();
  ev_prefix_kernel<<<nrec, 256, 0, st>>>(blk, none, nblk, pre, recs);
  AIR_CHECK_LAUNCH();
  int gy = EV_CURVE_WGS / nblk;
  gy = gy < 1 ? 1 : (gy > nrec ? nrec : gy);
  ev_curve_kernel<<<dim3(nblk, gy), EV_THREADS, 0, st>>>(keys, n, n_groups, pre, want_dcf ? 1 : 0, c12, c1, c2, recs, partial);
  AIR_CHECK_LAUNCH();
  ev_final_kernel<<<nrec, 256, 0, st>>>(partial, nblk, keys, want_dcf ? 1 : 0, recs);
  AIR_CHECK_LAUNCH();
  return AIR_OK;
}

// the whole chain behind both public entry points: n_groups + 1 records from one sort
int ev_det_min(const float* scores, const void* labels, int label_bytes, const void* groups, int group_bytes, int n,
               int n_groups, int negate, int want_dcf, const double* c12, double c1, double c2, air_eval_record* recs,
               void* ws, size_t ws_bytes, air_stream_t stream) {
  if (!scores || !labels || !recs || (label_bytes != 4 && label_bytes != 8)) return AIR_EINVAL;
  int rc = ev_check(n, n_groups, ws, ws_bytes);
  if (rc != AIR_OK) return rc;
  hipStream_t st = air_stream(stream);
  rc = ev_keys(scores, labels, label_bytes, groups, group_bytes, n, n_groups, negate, ws, st);
  if (rc != AIR_OK) return rc;
  rc = ev_sort(ws, n, st);  // once, whatever n_groups is
  if (rc != AIR_OK) return rc;
  return ev_curve_min(n, n_groups, want_dcf, c12, c1, c2, recs, ws, st);
}

}  // namespace

extern "C" {

int air_eval_max_trials(void) { return EV_MAX_N; }
int air_eval_sort_block(void) { return EV_BLOCK; }
int air_eval_max_groups(void) { return EV_MAX_GROUPS; }

size_t air_eval_workspace_bytes(int n) { return (n < 1 || n > EV_MAX_N) ? 0 : ev_bytes(n, 0); }

size_t air_eval_workspace_bytes_grouped(int n, int n_groups) {
  return (n < 1 || n > EV_MAX_N || n_groups < 1 || n_groups > EV_MAX_GROUPS) ? 0 : ev_bytes(n, n_groups);
}

int air_eval_det_min(const float* scores, const void* labels, int label_bytes, int n, int negate, int want_dcf, double c1,
                     double c2, air_eval_record* rec, void* ws, size_t ws_bytes, air_stream_t stream) {
  return ev_det_min(scores, labels, label_bytes, nullptr, 4, n, 0, negate, want_dcf, nullptr, c1, c2, rec, ws, ws_bytes, stream);
}

int air_eval_det_min_grouped(const float* scores, const void* labels, int label_bytes, const void* groups, int group_bytes,
                             int n, int n_groups, int negate, int want_dcf, const double* c12_dev, air_eval_record* recs,
                             void* ws, size_t ws_bytes, air_stream_t stream) {
  if (!groups || (group_bytes != 4 && group_bytes != 8) || (want_dcf && !c12_dev)) return AIR_EINVAL;
  // (zero groups is air_eval_det_min's call: here it is out of range like a negative count)
  return ev_det_min(scores, labels, label_bytes, groups, group_bytes, n, n_groups < 1 ? -1 : n_groups, negate, want_dcf,
                    want_dcf ? c12_dev : nullptr, 1.0, 1.0, recs, ws, ws_bytes, stream);
}

// the pooled chain step by step, on one workspace
int air_eval_keys(const float* scores, const void* labels, int label_bytes, int n, int negate, void* ws, size_t ws_bytes,
                  air_stream_t stream) {
  if (!scores || !labels || (label_bytes != 4 && label_bytes != 8)) return AIR_EINVAL;
  const int rc = ev_check(n, 0, ws, ws_bytes);
  return rc != AIR_OK ? rc : ev_keys(scores, labels, label_bytes, nullptr, 4, n, 0, negate, ws, air_stream(stream));
}

int air_eval_sort_keys(int n, void* ws, size_t ws_bytes, air_stream_t stream) {
  const int rc = ev_check(n, 0, ws, ws_bytes);
  return rc != AIR_OK ? rc : ev_sort(ws, n, air_stream(stream));
}

int air_eval_curve_min(int n, int want_dcf, double c1, double c2, air_eval_record* rec, void* ws, size_t ws_bytes,
                       air_stream_t stream) {
  if (!rec) return AIR_EINVAL;
  const int rc = ev_check(n, 0, ws, ws_bytes);
  return rc != AIR_OK ? rc : ev_curve_min(n, 0, want_dcf, nullptr, c1, c2, rec, ws, air_stream(stream));
}

}  // extern "C"
