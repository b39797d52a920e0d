// tokens.hip -- Phase B of encodeFrameParallel on the GPU, for methods 3-6
// without rate control (internal/lossy/encode.go:1356-1385): from the
// wg_mb_enc records wg_encode_mbs leaves on the device to the token stream a
// bool coder consumes, so the host copies tokens and 32-byte headers instead
// of 864-byte records and runs no serial pass over coefficients.
//
//   recordAllTokens / collectMBStats  internal/lossy/encode_parallel.go:1503-1707
//   collectCoeffStats / LevelStats    internal/lossy/encode_proba.go:10-113
//   optimizeProba, branchCost         encode_proba.go:117-168
//   recordMBTokens                    internal/lossy/encode_frame.go:647-759
//   RecordCoeffs, recordLevelVP8      internal/lossy/encode_token.go:115-300
//
// The reference records with the input probabilities and records again when
// optimizeProba changed one; the end state is one recording with the
// optimised table, which is what runs here.
//
// What makes the serial pass parallel: a coefficient's tokens depend only on
// its level, the previous level of its block (context 0 / 1 / 2 and whether an
// end-of-block test precedes), the block's non-zero count and the block's
// start context.  The start context of a Y or chroma block comes from the
// block above and the block to the left -- inside the MB, or the bottom row /
// right column of the neighbouring MB (0 when that MB is skipped or outside
// the frame).  Only the I16 DC context is carried: topNzDC[x] / leftNzDC are
// written by I16 MBs alone (a skipped one writes 0) and I4 MBs leave them, so
// the bit MB (x, y) sees is that of the nearest I16 MB above in its column /
// to its left in its row.  Launches, all on the caller's stream, none waiting
// on another workgroup:
//
//   k_tok_mbctx   one lane per MB: wg_mb_hdr's mode fields and a context word
//                 (the MB's bottom-row / right-column non-zero bits, its DC bit)
//   k_tok_dcwalk  one lane per MB column and per MB row: the carried DC bits
//   k_tok_count   one wave per MB, one lane per (block, zigzag position), four
//                 blocks a step: per-MB token counts and the 2112 counters, in
//                 an LDS histogram flushed with integer atomicAdd (sums of
//                 integers: order-independent, bit-exact)
//   k_tok_scan    per image: exclusive scan of the counts, skip statistics
//   k_tok_proba   per image: optimizeProba over the 1056 entries
//   k_tok_write   wg_encode_tokens: k_tok_count's mapping; a wave prefix sum of
//                 the lanes' token counts places them in an LDS stage that is
//                 stored to the stream as whole dwords
#include <stdint.h>

#include "vp8_tables.h"
#include "wg_common.h"

namespace {

constexpr int kRecBytes = 864;          // sizeof(wg_mb_enc)
constexpr int kRecVec = kRecBytes / 16; // uint4 loads per record
constexpr int kNumStats = 4 * 8 * 3 * 11 * 2;
constexpr int kNumProba = 4 * 8 * 3 * 11;
constexpr int kWaves = 4;               // waves per workgroup, one MB each at a time
constexpr int kMbPerWg = 64;            // MBs a workgroup of k_tok_count / k_tok_write walks
constexpr int kSteps = 7;               // 25 block slots, 4 a step
constexpr int kMaxLaneTokens = 19;      // p0, p1, 5 tree bits, 11 extra bits, sign
constexpr int kStageTokens = 64 * kMaxLaneTokens + 2;
constexpr uint32_t kMaxMbTokens = 25 * 16 * kMaxLaneTokens;

static_assert(sizeof(wg_mb_enc) == kRecBytes && sizeof(wg_mb_hdr) == 32 && sizeof(wg_token_summary) == 16, "ABI");

// record offsets (wg_mb_enc)
constexpr int kOffModes = 800, kOffNzY = 816, kOffNzUV = 832, kOffType = 848, kOffNzDC = 851, kOffSkip = 852;

// context word of an MB, as its lower and right neighbours read it
//   bits 0-3   Y blocks 12..15 (bottom row), 4-7 Y blocks 3, 7, 11, 15 (right column)
//   bits 8-9   U bottom, 10-11 U right, 12-13 V bottom, 14-15 V right
//   bit 16     the MB is I16 (it writes the DC context), bit 17 the DC bit it writes
__global__ void __launch_bounds__(256) k_tok_mbctx(const uint8_t* __restrict__ mb_enc, int64_t n_mb,
                                                    wg_mb_hdr* __restrict__ hdr, uint32_t* __restrict__ ctxw) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_mb) return;
  const uint4* rec = reinterpret_cast<const uint4*>(mb_enc + i * kRecBytes);
  const uint4 modes = rec[kOffModes / 16], nzy4 = rec[kOffNzY / 16], t2 = rec[kOffNzUV / 16], t3 = rec[kOffType / 16];
  const uint32_t mb_type = t3.x & 0xff, i16_mode = (t3.x >> 8) & 0xff, uv_mode = (t3.x >> 16) & 0xff, nz_dc = t3.x >> 24;
  const uint32_t skip = t3.y & 0xff, segment = (t3.y >> 8) & 0xff;
  uint4* h = reinterpret_cast<uint4*>(hdr + i);
  h[0] = modes;
  *reinterpret_cast<uint2*>(h + 1) = make_uint2(mb_type | (i16_mode << 8) | (uv_mode << 16) | (skip << 24), segment);
  const uint32_t i16 = mb_type == 0, first = i16;
  uint32_t w = 0;
  if (!skip) {
    const uint32_t nzy[4] = {nzy4.x, nzy4.y, nzy4.z, nzy4.w};
    for (int k = 0; k < 4; k++) {
      w |= (uint32_t)(((nzy[3] >> (8 * k)) & 0xff) > first) << k;        // blocks 12 + k
      w |= (uint32_t)((nzy[k] >> 24) > first) << (4 + k);                // blocks 4k + 3
    }
    const uint32_t uv[2] = {t2.x, t2.y};
    for (int ch = 0; ch < 2; ch++) {
      const uint32_t b0 = uv[ch] & 0xff, b1 = (uv[ch] >> 8) & 0xff, b2 = (uv[ch] >> 16) & 0xff, b3 = uv[ch] >> 24;
      (void)b0;
      w |= (uint32_t)(b2 > 0) << (8 + 4 * ch) | (uint32_t)(b3 > 0) << (9 + 4 * ch);
      w |= (uint32_t)(b1 > 0) << (10 + 4 * ch) | (uint32_t)(b3 > 0) << (11 + 4 * ch);
    }
    if (i16 && nz_dc > 0) w |= 1u << 17;
  }
  w |= i16 << 16;
  ctxw[i] = w;
}

// topNzDC / leftNzDC as MB (x, y) finds them: lanes [0, mbw) walk a column
// each, lanes [mbw, mbw + mbh) a row each.
__global__ void __launch_bounds__(256) k_tok_dcwalk(const uint32_t* __restrict__ ctxw, int mbw, int mbh,
                                                     uint8_t* __restrict__ dctop, uint8_t* __restrict__ dcleft) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int64_t base = (int64_t)blockIdx.y * mbw * mbh;
  if (t < mbw) {
    uint32_t carry = 0;
    for (int y = 0; y < mbh; y++) {
      const int64_t i = base + (int64_t)y * mbw + t;
      dctop[i] = (uint8_t)carry;
      const uint32_t w = ctxw[i];
      if (w & (1u << 16)) carry = (w >> 17) & 1;
    }
  } else if (t < mbw + mbh) {
    const int y = t - mbw;
    uint32_t carry = 0;
    for (int x = 0; x < mbw; x++) {
      const int64_t i = base + (int64_t)y * mbw + x;
      dcleft[i] = (uint8_t)carry;
      const uint32_t w = ctxw[i];
      if (w & (1u << 16)) carry = (w >> 17) & 1;
    }
  }
}

// What one lane emits: the tokens of zigzag position n of one block.
struct LaneWork {
  int active;  // emits anything
  int tbc;     // (type * 8 + band) * 3 + ctx
  int eob;     // the end-of-block token only
  int p0;      // a not-end-of-block token precedes
  int v;       // the level
};

// Block slot `slot` (0: the I16 DC block, 1..16: Y blocks, 17..24: U then V
// blocks -- recordMBTokens' order) of the record at `rec` (LDS), position n =
// lane & 15.  Called by the whole wave (it ballots).  The end of a block is
// found as RecordCoeffs finds it: the end-of-block test runs at the first
// position and after every non-zero level, and ends the block at the first of
// those at or past the record's non-zero count.
__device__ __forceinline__ LaneWork lane_work(const uint8_t* rec, int slot, int lane, uint32_t topw, uint32_t leftw,
                                              uint32_t dc_ctx) {
  LaneWork lw;
  const int n = lane & 15, g = lane >> 4;
  const int16_t* coeffs = reinterpret_cast<const int16_t*>(rec);
  const int i16 = rec[kOffType] == 0, skip = rec[kOffSkip] != 0;
  const bool valid = slot < 25 && !skip && (slot > 0 || i16);
  int type = 1, first = 0, nz = 0, base = 384, c0 = (int)dc_ctx;
  if (valid && slot >= 17) {
    const int k = slot - 17, ch = k >> 2, ux = k & 1, uy = (k >> 1) & 1;
    type = 2;
    base = (16 + k) * 16;
    nz = rec[kOffNzUV + k];
    const int top = uy ? rec[kOffNzUV + k - 2] > 0 : (int)((topw >> (8 + 4 * ch + ux)) & 1);
    const int left = ux ? rec[kOffNzUV + k - 1] > 0 : (int)((leftw >> (10 + 4 * ch + uy)) & 1);
    c0 = top + left;
  } else if (valid && slot >= 1) {
    const int b = slot - 1, bx = b & 3, by = b >> 2;
    type = i16 ? 0 : 3;
    first = i16;
    base = b * 16;
    nz = rec[kOffNzY + b];
    const int top = by ? rec[kOffNzY + b - 4] > first : (int)((topw >> bx) & 1);
    const int left = bx ? rec[kOffNzY + b - 1] > first : (int)((leftw >> (4 + by)) & 1);
    c0 = top + left;
  } else if (valid) {
    nz = rec[kOffNzDC];
  }
  const int v = valid ? coeffs[base + vp8_zigzag[n]] : 0;
  const unsigned long long bal = __ballot(v != 0 && n >= first);
  const uint32_t m = (uint32_t)(bal >> (16 * g)) & 0xffffu;
  const uint32_t tests = ((m << 1) | (1u << first)) & 0xffffu;  // positions where the end-of-block test runs
  const int lo = nz > first ? nz : first;
  const uint32_t cand = lo >= 16 ? 0u : tests & ~((1u << lo) - 1u);
  const int end = cand ? __builtin_ctz(cand) : 16;
  int ctx = c0;
  if (n > first) {
    const int prev = coeffs[base + vp8_zigzag[n - 1]];
    ctx = prev == 0 ? 0 : ((prev == 1 || prev == -1) ? 1 : 2);
  }
  lw.active = valid && n >= first && n <= end;
  lw.tbc = (type * 8 + vp8_bands[n]) * 3 + ctx;
  lw.eob = n == end;
  lw.p0 = (tests >> n) & 1;
  lw.v = v;
  return lw;
}

// RecordCoeffs' body for one position + recordLevelVP8 (encode_token.go:139-300;
// the same branches as collectCoeffStats / collectLevelStats).  S::tok(p, bit):
// a token priced by probability p of the lane's (type, band, ctx);
// S::fixed(bit, prob): one with a fixed probability.
template <class S>
__device__ __forceinline__ void walk_tokens(const LaneWork& lw, S& s) {
  if (lw.eob) {
    s.tok(0, 0);
    return;
  }
  if (lw.p0) s.tok(0, 1);
  const int sign = lw.v < 0;
  const int level = sign ? -lw.v : lw.v;
  if (level == 0) {
    s.tok(1, 0);
    return;
  }
  s.tok(1, 1);
  if (level == 1) {
    s.tok(2, 0);
  } else {
    s.tok(2, 1);
    if (level <= 4) {
      s.tok(3, 0);
      if (level == 2) {
        s.tok(4, 0);
      } else {
        s.tok(4, 1);
        s.tok(5, level == 4);
      }
    } else if (level <= 10) {
      s.tok(3, 1);
      s.tok(6, 0);
      if (level <= 6) {
        s.tok(7, 0);
        s.fixed(level - 5, 159);
      } else {
        s.tok(7, 1);
        s.fixed((level - 7) >> 1, 165);
        s.fixed((level - 7) & 1, 145);
      }
    } else {
      s.tok(3, 1);
      s.tok(6, 1);
      const int cat = level <= 18 ? 0 : (level <= 34 ? 1 : (level <= 66 ? 2 : 3));
      const int bit1 = cat >> 1, bit0 = cat & 1;
      s.tok(8, bit1);
      s.tok(9 + bit1, bit0);
      const int extra = level - (3 + (8 << cat));
      const uint8_t* tab = cat == 0 ? vp8_cat3 : (cat == 1 ? vp8_cat4 : (cat == 2 ? vp8_cat5 : vp8_cat6));
      const int nbits = cat == 0 ? 3 : (cat == 1 ? 4 : (cat == 2 ? 5 : 11));
      for (int i = 0; i < nbits; i++) s.fixed((extra >> (nbits - 1 - i)) & 1, tab[i]);
    }
  }
  s.fixed(sign, 128);
}

struct CountSink {
  uint32_t* hist;  // LDS, this lane's (type, band, ctx) row: [11][2]
  int count;
  __device__ __forceinline__ void tok(int p, int bit) {
    atomicAdd(&hist[2 * p + bit], 1u);
    count++;
  }
  __device__ __forceinline__ void fixed(int, int) { count++; }
};

struct Counter {
  int n;
  __device__ __forceinline__ void tok(int, int) { n++; }
  __device__ __forceinline__ void fixed(int, int) { n++; }
};

struct WriteSink {
  const uint8_t* proba;  // LDS, this lane's (type, band, ctx) row: [11]
  uint16_t* out;         // LDS stage
  __device__ __forceinline__ void tok(int p, int bit) { *out++ = (uint16_t)(bit | (proba[p] << 8)); }
  __device__ __forceinline__ void fixed(int bit, int prob) { *out++ = (uint16_t)(bit | (prob << 8)); }
};

__device__ __forceinline__ int wave_sum(int v) {
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
  return v;
}
__device__ __forceinline__ int wave_inclusive_scan(int v, int lane) {
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(v, d);
    if (lane >= d) v += o;
  }
  return v;
}

// The neighbours' context of MB (x, y) of an image (wave-uniform loads).
__device__ __forceinline__ void neighbour_ctx(const uint32_t* ctxw, const uint8_t* dctop, const uint8_t* dcleft,
                                              int64_t gi, int x, int y, int mbw, uint32_t* topw, uint32_t* leftw,
                                              uint32_t* dc_ctx) {
  *topw = y > 0 ? ctxw[gi - mbw] : 0u;
  *leftw = x > 0 ? ctxw[gi - 1] : 0u;
  *dc_ctx = (uint32_t)dctop[gi] + (uint32_t)dcleft[gi];
}

// Every wave of the workgroup runs the same number of loop passes (a wave
// past the image's last MB idles through them), so the barriers are uniform.
__global__ void __launch_bounds__(64 * kWaves) k_tok_count(const uint8_t* __restrict__ mb_enc, int mbw, int mbh,
                                                           const uint32_t* __restrict__ ctxw,
                                                           const uint8_t* __restrict__ dctop,
                                                           const uint8_t* __restrict__ dcleft,
                                                           wg_mb_hdr* __restrict__ hdr, uint32_t* __restrict__ stats) {
  __shared__ uint32_t hist[kNumStats];
  __shared__ uint4 recs[kWaves][kRecVec];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n_mb = mbw * mbh;
  const int64_t img_base = (int64_t)blockIdx.y * n_mb;
  for (int i = tid; i < kNumStats; i += 64 * kWaves) hist[i] = 0;
  for (int pass = 0; pass < kMbPerWg / kWaves; pass++) {
    const int mb = blockIdx.x * kMbPerWg + pass * kWaves + wave;
    const bool have = mb < n_mb;
    const int64_t gi = img_base + (have ? mb : 0);
    __syncthreads();  // the previous pass is done with recs (and hist is zeroed)
    if (have && lane < kRecVec) recs[wave][lane] = reinterpret_cast<const uint4*>(mb_enc + gi * kRecBytes)[lane];
    __syncthreads();
    if (!have) continue;
    uint32_t topw, leftw, dc_ctx;
    neighbour_ctx(ctxw, dctop, dcleft, gi, mb % mbw, mb / mbw, mbw, &topw, &leftw, &dc_ctx);
    const uint8_t* rec = reinterpret_cast<const uint8_t*>(recs[wave]);
    int count = 0;
    for (int step = 0; step < kSteps; step++) {
      const LaneWork lw = lane_work(rec, step * 4 + (lane >> 4), lane, topw, leftw, dc_ctx);
      if (lw.active) {
        CountSink s{hist + lw.tbc * 22, 0};
        walk_tokens(lw, s);
        count += s.count;
      }
    }
    count = wave_sum(count);
    if (lane == 0) hdr[gi].tok_count = (uint32_t)count;
  }
  __syncthreads();
  uint32_t* out = stats + (int64_t)blockIdx.y * kNumStats;
  for (int i = tid; i < kNumStats; i += 64 * kWaves) {
    const uint32_t c = hist[i];
    if (c) atomicAdd(&out[i], c);
  }
}

// Exclusive scan of tok_count in raster order, the skip count and skipProba
// (encode_parallel.go:1595-1597); one workgroup per image.
__global__ void __launch_bounds__(256) k_tok_scan(wg_mb_hdr* __restrict__ hdr, int n_mb,
                                                  wg_token_summary* __restrict__ summary) {
  __shared__ uint32_t part[256], skips[256];
  const int tid = threadIdx.x;
  wg_mb_hdr* h = hdr + (int64_t)blockIdx.x * n_mb;
  const int per = (n_mb + 255) / 256;
  const int lo = tid * per < n_mb ? tid * per : n_mb;
  const int hi = lo + per < n_mb ? lo + per : n_mb;
  uint32_t sum = 0, nskip = 0;
  for (int i = lo; i < hi; i++) {
    sum += h[i].tok_count;
    nskip += h[i].skip != 0;
  }
  part[tid] = sum;
  skips[tid] = nskip;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {  // inclusive scan of the 256 partial sums
    const uint32_t a = tid >= d ? part[tid - d] : 0, b = tid >= d ? skips[tid - d] : 0;
    __syncthreads();
    part[tid] += a;
    skips[tid] += b;
    __syncthreads();
  }
  uint32_t run = part[tid] - sum;
  for (int i = lo; i < hi; i++) {
    h[i].tok_start = run;
    run += h[i].tok_count;
  }
  if (tid == 255) {
    const uint32_t total_skip = skips[255];
    wg_token_summary s;
    s.total_tokens = part[255];
    s.num_skip = total_skip;
    s.num_updates = 0;  // k_tok_proba
    s.skip_proba = total_skip ? (uint8_t)(((uint32_t)n_mb - total_skip) * 255u / (uint32_t)n_mb) : 0;
    s.pad[0] = s.pad[1] = s.pad[2] = 0;
    summary[blockIdx.x] = s;
  }
}

// VP8BitCost (internal/dsp/cost.go:43-48)
__device__ __forceinline__ int64_t bit_cost(int bit, int p) { return vp8_entropy_cost[bit ? 255 - p : p]; }
// branchCost (encode_proba.go:160-168); Go's int is 64 bits
__device__ __forceinline__ int64_t branch_cost(int64_t cnt0, int64_t cnt1, int p) {
  p = p < 1 ? 1 : (p > 255 ? 255 : p);
  return cnt1 * bit_cost(1, p) + cnt0 * bit_cost(0, p);
}

// optimizeProba (encode_proba.go:117-156); one workgroup per image.
__global__ void __launch_bounds__(256) k_tok_proba(const uint32_t* __restrict__ stats,
                                                   const uint8_t* __restrict__ proba_in, int64_t proba_in_pitch,
                                                   uint8_t* __restrict__ proba_out,
                                                   wg_token_summary* __restrict__ summary) {
  __shared__ int updates[256];
  const int tid = threadIdx.x;
  const uint32_t* st = stats + (int64_t)blockIdx.x * kNumStats;
  const uint8_t* pin = proba_in + (int64_t)blockIdx.x * proba_in_pitch;
  uint8_t* pout = proba_out + (int64_t)blockIdx.x * kNumProba;
  int n = 0;
  for (int k = tid; k < kNumProba; k += 256) {
    const int64_t cnt0 = st[2 * k], cnt1 = st[2 * k + 1], total = cnt0 + cnt1;
    uint8_t p = pin[k];
    if (total > 0) {
      const int new_p = cnt1 > 0 ? (int)(255 - cnt1 * 255 / total) : 255;
      const int upd = vp8_coeffs_update_proba[k];
      const int64_t old_cost = branch_cost(cnt0, cnt1, vp8_coeffs_proba0[k]) + bit_cost(0, upd);
      const int64_t new_cost = branch_cost(cnt0, cnt1, new_p) + bit_cost(1, upd) + 8 * 256;
      if (old_cost > new_cost) {
        p = (uint8_t)new_p;
        n++;
      }
    }
    pout[k] = p;
  }
  updates[tid] = n;
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if (tid < d) updates[tid] += updates[tid + d];
    __syncthreads();
  }
  if (tid == 0) summary[blockIdx.x].num_updates = (uint32_t)updates[0];
}

// wg_encode_tokens.  Per step a wave stages the tokens of four blocks in LDS
// at the parity of their place in the stream, so that LDS dword k is stream
// dword k of the step: whole dwords are stored, and only a first / last token
// that shares its dword with another step (or MB) goes out as 2 bytes.
__global__ void __launch_bounds__(64 * kWaves) k_tok_write(const uint8_t* __restrict__ mb_enc, int mbw, int mbh,
                                                           const uint32_t* __restrict__ ctxw,
                                                           const uint8_t* __restrict__ dctop,
                                                           const uint8_t* __restrict__ dcleft,
                                                           const wg_mb_hdr* __restrict__ hdr,
                                                           const uint8_t* __restrict__ proba, uint8_t* __restrict__ tokens,
                                                           int64_t tokens_pitch) {
  __shared__ uint4 recs[kWaves][kRecVec];
  __shared__ __attribute__((aligned(4))) uint16_t stage[kWaves][kStageTokens];
  __shared__ uint8_t prob[kNumProba];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n_mb = mbw * mbh;
  const int64_t img_base = (int64_t)blockIdx.y * n_mb;
  for (int i = tid; i < kNumProba; i += 64 * kWaves) prob[i] = proba[(int64_t)blockIdx.y * kNumProba + i];
  uint8_t* img_tokens = tokens + (int64_t)blockIdx.y * tokens_pitch;
  for (int pass = 0; pass < kMbPerWg / kWaves; pass++) {
    const int mb = blockIdx.x * kMbPerWg + pass * kWaves + wave;
    const bool have = mb < n_mb;
    const int64_t gi = img_base + (have ? mb : 0);
    __syncthreads();
    if (have && lane < kRecVec) recs[wave][lane] = reinterpret_cast<const uint4*>(mb_enc + gi * kRecBytes)[lane];
    __syncthreads();
    uint32_t topw = 0, leftw = 0, dc_ctx = 0;
    int64_t pos = 0, mb_end = 0;
    bool fits = false;
    if (have) {
      neighbour_ctx(ctxw, dctop, dcleft, gi, mb % mbw, mb / mbw, mbw, &topw, &leftw, &dc_ctx);
      pos = hdr[gi].tok_start;
      mb_end = pos + hdr[gi].tok_count;
      fits = 2 * mb_end <= tokens_pitch;  // an MB whose range passes the image's buffer writes nothing
    }
    const uint8_t* rec = reinterpret_cast<const uint8_t*>(recs[wave]);
    uint16_t* st = stage[wave];
    for (int step = 0; step < kSteps; step++) {
      int count = 0, total = 0, par = 0;
      if (have) {  // wave-uniform
        const LaneWork lw = lane_work(rec, step * 4 + (lane >> 4), lane, topw, leftw, dc_ctx);
        if (lw.active) {
          Counter cnt{0};
          walk_tokens(lw, cnt);
          count = cnt.n;
        }
        const int incl = wave_inclusive_scan(count, lane);
        total = __shfl(incl, 63);
        par = (int)(pos & 1);
        if (lw.active) {
          WriteSink w{prob + lw.tbc * 11, st + par + incl - count};
          walk_tokens(lw, w);
        }
      }
      __syncthreads();  // the stage is written
      // never past the count the scan reserved for this MB (records are the same, so total fits; the guard keeps
      // a record changed between the two calls from writing outside its range)
      if (have && fits && total > 0 && pos + total <= mb_end) {
        const int last = par + total;  // stage tokens [par, last)
        uint8_t* dst = img_tokens + 2 * (pos - par);  // stream address of stage token 0: 4-byte aligned
        if (par && lane == 0) *reinterpret_cast<uint16_t*>(dst + 2) = st[1];
        const int d0 = par ? 1 : 0, d1 = last >> 1;  // whole dwords [d0, d1)
        const uint32_t* st32 = reinterpret_cast<const uint32_t*>(st);
        for (int d = d0 + lane; d < d1; d += 64) reinterpret_cast<uint32_t*>(dst)[d] = st32[d];
        if ((last & 1) && lane == 63)  // not the head token: par = 1 with an odd `last` has total >= 2
          *reinterpret_cast<uint16_t*>(dst + 2 * (last - 1)) = st[last - 1];
      }
      pos += total;
      __syncthreads();  // the stage is read
    }
  }
}

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

struct WorkLayout {
  size_t ctxw, dctop, dcleft, stats, total;
};
WorkLayout work_layout(int64_t n_mb_all, int n_images) {
  WorkLayout w;
  w.ctxw = 0;
  w.dctop = align16((size_t)n_mb_all * 4);
  w.dcleft = w.dctop + align16((size_t)n_mb_all);
  w.stats = w.dcleft + align16((size_t)n_mb_all);
  w.total = w.stats + (size_t)n_images * kNumStats * sizeof(uint32_t);
  return w;
}

bool shape_ok(int32_t mbw, int32_t mbh, int32_t n_images) {
  return mbw > 0 && mbh > 0 && n_images > 0 && n_images <= 65535 &&
         (uint64_t)mbw * (uint64_t)mbh * kMaxMbTokens <= 0xffffffffull &&
         (uint64_t)mbw * (uint64_t)mbh * (uint64_t)n_images <= 0x7fffffffull;
}

}  // namespace

extern "C" size_t wg_encode_tokens_work_bytes(int32_t mbw, int32_t mbh, int32_t n_images) {
  if (!shape_ok(mbw, mbh, n_images)) return 0;
  return work_layout((int64_t)mbw * mbh * n_images, n_images).total;
}

// The context arrays of one call: k_tok_mbctx + k_tok_dcwalk into `ctx`.
static int build_contexts(const void* mb_enc, int32_t mbw, int32_t mbh, int32_t n_images, wg_mb_hdr* hdr, uint8_t* ctx,
                          hipStream_t s) {
  const int64_t n_all = (int64_t)mbw * mbh * n_images;
  const WorkLayout L = work_layout(n_all, n_images);
  uint32_t* ctxw = reinterpret_cast<uint32_t*>(ctx + L.ctxw);
  hipLaunchKernelGGL(k_tok_mbctx, dim3(wg::blocks_for(n_all, 256)), dim3(256), 0, s,
                     static_cast<const uint8_t*>(mb_enc), n_all, hdr, ctxw);
  hipLaunchKernelGGL(k_tok_dcwalk, dim3(wg::blocks_for(mbw + mbh, 256), (unsigned)n_images), dim3(256), 0, s, ctxw, mbw,
                     mbh, ctx + L.dctop, ctx + L.dcleft);
  return wg::check_launch("wg_encode_token_stats (contexts)");
}

extern "C" int wg_encode_token_stats(const void* mb_enc, int32_t mbw, int32_t mbh, int32_t n_images,
                                     const uint8_t* proba_in, int64_t proba_in_pitch, uint32_t* stats,
                                     uint8_t* proba_out, wg_mb_hdr* hdr, wg_token_summary* summary, void* work,
                                     void* stream) {
  WG_REQUIRE(mb_enc && proba_in && proba_out && hdr && summary && work);
  WG_REQUIRE(shape_ok(mbw, mbh, n_images));
  WG_REQUIRE(proba_in_pitch == 0 || proba_in_pitch >= kNumProba);
  WG_REQUIRE(((uintptr_t)mb_enc & 15) == 0 && ((uintptr_t)hdr & 15) == 0 && ((uintptr_t)work & 15) == 0);
  WG_REQUIRE(((uintptr_t)summary & 3) == 0 && ((uintptr_t)stats & 3) == 0);
  hipStream_t s = wg::as_stream(stream);
  const int64_t n_all = (int64_t)mbw * mbh * n_images;
  const WorkLayout L = work_layout(n_all, n_images);
  uint8_t* w = static_cast<uint8_t*>(work);
  uint32_t* st = stats ? stats : reinterpret_cast<uint32_t*>(w + L.stats);
  if (hipMemsetAsync(st, 0, (size_t)n_images * kNumStats * sizeof(uint32_t), s) != hipSuccess)
    return wg::check_launch("wg_encode_token_stats (clear)");
  const int rc = build_contexts(mb_enc, mbw, mbh, n_images, hdr, w, s);
  if (rc != WG_OK) return rc;
  const unsigned groups = wg::blocks_for((int64_t)mbw * mbh, kMbPerWg);
  hipLaunchKernelGGL(k_tok_count, dim3(groups, (unsigned)n_images), dim3(64 * kWaves), 0, s,
                     static_cast<const uint8_t*>(mb_enc), mbw, mbh, reinterpret_cast<const uint32_t*>(w + L.ctxw),
                     w + L.dctop, w + L.dcleft, hdr, st);
  hipLaunchKernelGGL(k_tok_scan, dim3((unsigned)n_images), dim3(256), 0, s, hdr, mbw * mbh, summary);
  hipLaunchKernelGGL(k_tok_proba, dim3((unsigned)n_images), dim3(256), 0, s, st, proba_in, proba_in_pitch, proba_out,
                     summary);
  return wg::check_launch("wg_encode_token_stats");
}

extern "C" int wg_encode_tokens(const void* mb_enc, int32_t mbw, int32_t mbh, int32_t n_images, const uint8_t* proba,
                                const wg_mb_hdr* hdr, const void* work, uint8_t* tokens, int64_t tokens_pitch,
                                void* stream) {
  WG_REQUIRE(mb_enc && proba && hdr && work);
  WG_REQUIRE(shape_ok(mbw, mbh, n_images));
  WG_REQUIRE(tokens_pitch >= 0 && (tokens_pitch & 3) == 0 && (tokens || tokens_pitch == 0));
  WG_REQUIRE(((uintptr_t)mb_enc & 15) == 0 && ((uintptr_t)work & 15) == 0 && ((uintptr_t)tokens & 3) == 0);
  if (tokens_pitch == 0) return WG_OK;  // no MB with tokens fits
  hipStream_t s = wg::as_stream(stream);
  const WorkLayout L = work_layout((int64_t)mbw * mbh * n_images, n_images);
  const uint8_t* w = static_cast<const uint8_t*>(work);
  const unsigned groups = wg::blocks_for((int64_t)mbw * mbh, kMbPerWg);
  hipLaunchKernelGGL(k_tok_write, dim3(groups, (unsigned)n_images), dim3(64 * kWaves), 0, s,
                     static_cast<const uint8_t*>(mb_enc), mbw, mbh, reinterpret_cast<const uint32_t*>(w + L.ctxw),
                     w + L.dctop, w + L.dcleft, hdr, proba, tokens, tokens_pitch);
  return wg::check_launch("wg_encode_tokens");
}
