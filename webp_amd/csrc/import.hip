// import.hip -- RGBA -> padded YUV420 planes for the VP8 encoder on gfx950
// (replaces VP8Encoder.importImage, internal/lossy/encode.go:671-943, the
// direct-pixel paths with and without dithering; arithmetic of
// internal/dsp/yuv.go, VP8Random of internal/dsp/random.go).
//
// Dithering (Preprocessing bit 1, encode.go:690-695, :793-809, :903-940):
// the reference draws one VP8Random value per padded pixel for Y in raster
// order, then two per chroma pixel (U, V) row pair by row pair, from a
// generator seeded identically for every image.  The stream therefore
// depends only on the padded frame size: wg_dither_plan runs the generator
// once on the host and leaves the draws in device memory (Y as int16, U/V as
// int32, 4 B per pixel), and the import kernel reads each pixel's draw next
// to its RGBA -- a per-size noise table instead of a serial generator.
//
// Streaming kernel: one thread per 2 rows x 4 columns of the padded frame
// (two 2x2 chroma quads), walking 8 row pairs.  Reads 2x16 B of RGBA, writes
// 2x4 B of Y and 2 B each of U and V per row pair.  Gamma tables (yuv.go:193-215) are built on the host with
// float64 pow, passed in the kernel argument block and staged in LDS.
// Padding replicates the last column / row exactly as the reference's clamp.
//
// k_import_ycbcr (further down) is the other way into the encoder's planes:
// VP8Encoder.importYCbCr (encode.go:544-585), the padding alone, for planes
// SharpYUV made (webp.Encode's UseSharpYUV).
#include <math.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "wg_common.h"
#include "wg_dsp.h"
#include "wg_yuv.h"

namespace {
using namespace wg;

// One 2x2 quad: gamma-correct (alpha-weighted when 0 < sum(A) < 1020) average
// of R, G, B, then RGBToU / RGBToV on the sum-of-4 values.  Returns u | v << 8.
__device__ __forceinline__ uint32_t quad_uv(const uint32_t* tl, const uint32_t* tg, uint32_t p0, uint32_t p1,
                                         uint32_t p2, uint32_t p3, int has_alpha, int rnd_u = 1 << 17,
                                         int rnd_v = 1 << 17) {
  const uint32_t a0 = has_alpha ? p0 >> 24 : 255u, a1 = has_alpha ? p1 >> 24 : 255u;
  const uint32_t a2 = has_alpha ? p2 >> 24 : 255u, a3 = has_alpha ? p3 >> 24 : 255u;
  const uint32_t ta = a0 + a1 + a2 + a3;
  const bool plain = (ta == 4 * 255) || (ta == 0);
  const uint32_t inv = plain ? 0u : (1u << 19) / ta;  // kInvAlpha[ta], yuv.go:343-447
  int c3[3];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const int sh = 8 * c;
    const uint32_t l0 = tl[(p0 >> sh) & 0xff], l1 = tl[(p1 >> sh) & 0xff];
    const uint32_t l2 = tl[(p2 >> sh) & 0xff], l3 = tl[(p3 >> sh) & 0xff];
    const uint32_t sum = plain ? l0 + l1 + l2 + l3 : ((a0 * l0 + a1 * l1 + a2 * l2 + a3 * l3) * inv) >> 17;
    c3[c] = lin_to_gamma(tg, sum, 0);
  }
  int u = clip_uv(-9719 * c3[0] - 19081 * c3[1] + 28800 * c3[2], rnd_u);
  int v = clip_uv(28800 * c3[0] - 24116 * c3[1] - 4684 * c3[2], rnd_v);
  // Keep the two clamps separate: hipcc (ROCm 7.2) otherwise fuses
  // "sat_u8(x>>18) | sat_u8(y>>18)<<8" into v_ashr_pk_u8_i32 and then assumes
  // the upper 16 bits of that result are zero, which the hardware does not
  // guarantee -- V picked up stray bits.  (Found by the parity tests.)
  asm volatile("" : "+v"(u));
  asm volatile("" : "+v"(v));
  return (uint32_t)u | ((uint32_t)v << 8);
}

struct ImportArgs {
  const uint8_t* rgba;
  uint8_t *y, *u, *v;
  int64_t rgba_pitch, y_pitch, uv_pitch;
  int w, h, stride, has_alpha, padw, padh;
  int chunks;    // padw / 4: 4-pixel chunks per row
  int pairs;     // n_images * padh / 2 row pairs in the batch
  int rp;        // row pairs walked per block (>= IM_RP; grid.y stays <= 65535)
  int aligned;   // rows start 16-byte aligned -> one 16 B load per row and chunk
  int amp;       // VP8Random amplitude (dithered variant)
  const int16_t* dither_y;   // [padh][padw] RandomBits(16) draws before scaling
  const int32_t* dither_uv;  // [padh/2][padw] RandomBits(18) draws, U and V interleaved
  GammaTabs tabs;
};

constexpr int IM_T = 256;   // threads per block: 256 chunks = 1024 columns of a row pair
constexpr int IM_RP = 8;    // minimum row pairs walked per block (amortises the table fill)

// Thread = one 4-pixel chunk of a row pair (two 2x2 chroma quads).  Lane i of
// a wave loads bytes [16i, 16i + 16) of each of the two RGBA rows, so every
// load instruction is one contiguous 1 KB span, and stores 4 B of Y per row
// and 2 B each of U and V (contiguous 256 B / 128 B per wave instruction).
// RandomBits2's scaling of a draw (random.go:68-70): (d * amp) >> 8 + half
__device__ __forceinline__ int dither_round(int d, int amp, int half) { return ((d * amp) >> 8) + half; }

template <bool DITHER>
__global__ __launch_bounds__(IM_T) void k_import(const ImportArgs a) {
  __shared__ uint32_t tl[256];
  __shared__ uint32_t tg[34];
  for (int i = threadIdx.x; i < 256; i += IM_T) tl[i] = a.tabs.to_lin[i];
  if (threadIdx.x < 34) tg[threadIdx.x] = a.tabs.to_gamma[threadIdx.x];
  __syncthreads();
  const int cx = blockIdx.x * IM_T + threadIdx.x;
  if (cx >= a.chunks) return;
  const int x0 = 4 * cx;
  const bool fast = a.aligned && x0 + 4 <= a.w;
  const int hp = a.padh >> 1;
  const int pair_end = min((int)(blockIdx.y + 1) * a.rp, a.pairs);
  for (int pr = blockIdx.y * a.rp; pr < pair_end; pr++) {
    const int img = pr / hp, yp = pr - img * hp;
    const uint8_t* src = a.rgba + img * a.rgba_pitch;
    uint32_t px[2][4];
#pragma unroll
    for (int r = 0; r < 2; r++) {
      const uint8_t* row = src + (int64_t)min(2 * yp + r, a.h - 1) * a.stride;
      if (fast) {
        const uint4 q = *reinterpret_cast<const uint4*>(row + 4 * x0);
        px[r][0] = q.x; px[r][1] = q.y; px[r][2] = q.z; px[r][3] = q.w;
      } else {
#pragma unroll
        for (int i = 0; i < 4; i++) px[r][i] = *reinterpret_cast<const uint32_t*>(row + 4 * min(x0 + i, a.w - 1));
      }
    }
    // Y (encode.go:757-793; dithered: RGBToYRounding with RandomBits(16), :793-809)
    int dy[2][4] = {{1 << 15, 1 << 15, 1 << 15, 1 << 15}, {1 << 15, 1 << 15, 1 << 15, 1 << 15}};
    int duv[4] = {1 << 17, 1 << 17, 1 << 17, 1 << 17};
    if (DITHER) {
#pragma unroll
      for (int r = 0; r < 2; r++) {
        const uint2 q = *reinterpret_cast<const uint2*>(a.dither_y + (int64_t)(2 * yp + r) * a.padw + x0);
        dy[r][0] = dither_round((int16_t)(q.x & 0xffff), a.amp, 1 << 15);
        dy[r][1] = dither_round((int16_t)(q.x >> 16), a.amp, 1 << 15);
        dy[r][2] = dither_round((int16_t)(q.y & 0xffff), a.amp, 1 << 15);
        dy[r][3] = dither_round((int16_t)(q.y >> 16), a.amp, 1 << 15);
      }
      const int4 q = *reinterpret_cast<const int4*>(a.dither_uv + (int64_t)yp * a.padw + x0);
      duv[0] = dither_round(q.x, a.amp, 1 << 17);
      duv[1] = dither_round(q.y, a.amp, 1 << 17);
      duv[2] = dither_round(q.z, a.amp, 1 << 17);
      duv[3] = dither_round(q.w, a.amp, 1 << 17);
    }
#pragma unroll
    for (int r = 0; r < 2; r++) {
      uint32_t yw = 0;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const uint32_t p = px[r][i];
        const int yv = DITHER ? (16839 * (int)(p & 0xff) + 33059 * (int)((p >> 8) & 0xff) + 6420 * (int)((p >> 16) & 0xff) +
                                 dy[r][i] + (16 << 16)) >> 16
                              : rgb_to_y(p & 0xff, (p >> 8) & 0xff, (p >> 16) & 0xff);
        yw |= (uint32_t)(yv & 0xff) << (8 * i);
      }
      *reinterpret_cast<uint32_t*>(a.y + img * a.y_pitch + (int64_t)(2 * yp + r) * a.padw + x0) = yw;
    }
    // U/V: AccumulateRGBA (yuv.go:486-517) + ConvertRGBA32ToUV (:553-562) or
    // ConvertRGBA32ToUVDithered (:568-576)
    const uint32_t uv0 = quad_uv(tl, tg, px[0][0], px[0][1], px[1][0], px[1][1], a.has_alpha, duv[0], duv[1]);
    const uint32_t uv1 = quad_uv(tl, tg, px[0][2], px[0][3], px[1][2], px[1][3], a.has_alpha, duv[2], duv[3]);
    const int64_t co = img * a.uv_pitch + (int64_t)yp * (a.padw >> 1) + (x0 >> 1);
    *reinterpret_cast<uint16_t*>(a.u + co) = (uint16_t)((uv0 & 0xff) | ((uv1 & 0xff) << 8));
    *reinterpret_cast<uint16_t*>(a.v + co) = (uint16_t)((uv0 >> 8) | (uv1 & 0xff00));
  }
}

}  // namespace

namespace {
int launch_import(const uint8_t* rgba, int32_t w, int32_t h, int32_t stride, int64_t rgba_pitch, int32_t has_alpha,
                  uint8_t* y, uint8_t* u, uint8_t* v, int64_t y_pitch, int64_t uv_pitch, int32_t n_images, int amp,
                  const void* plan, void* stream) {
  WG_REQUIRE(rgba && y && u && v);
  WG_REQUIRE(w > 0 && h > 0 && n_images > 0 && stride >= 4 * w && (stride & 3) == 0);
  WG_REQUIRE((reinterpret_cast<uintptr_t>(rgba) & 3) == 0 && (rgba_pitch & 3) == 0);
  const int mbw = (w + 15) >> 4, mbh = (h + 15) >> 4;
  WG_REQUIRE(((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(u) | reinterpret_cast<uintptr_t>(v)) &
              3) == 0 && (y_pitch & 7) == 0 && (uv_pitch & 3) == 0);
  WG_REQUIRE(y_pitch >= (int64_t)256 * mbw * mbh && uv_pitch >= (int64_t)64 * mbw * mbh);
  ImportArgs a;
  a.rgba = rgba;
  a.y = y;
  a.u = u;
  a.v = v;
  a.rgba_pitch = rgba_pitch;
  a.y_pitch = y_pitch;
  a.uv_pitch = uv_pitch;
  a.w = w;
  a.h = h;
  a.stride = stride;
  a.has_alpha = has_alpha ? 1 : 0;
  a.padw = 16 * mbw;
  a.padh = 16 * mbh;
  a.chunks = a.padw / 4;
  WG_REQUIRE((int64_t)n_images * (a.padh / 2) < (1ll << 31) / 2);
  a.pairs = n_images * (a.padh / 2);
  a.tabs = host_tabs();
  a.aligned = ((reinterpret_cast<uintptr_t>(rgba) | (uintptr_t)stride | (uintptr_t)rgba_pitch) & 15) == 0;
  a.rp = max(IM_RP, (int)wg::blocks_for(a.pairs, 65535));
  a.amp = amp;
  a.dither_y = static_cast<const int16_t*>(plan);
  a.dither_uv = plan ? reinterpret_cast<const int32_t*>(static_cast<const int16_t*>(plan) + (int64_t)a.padw * a.padh)
                     : nullptr;
  const dim3 grid(wg::blocks_for(a.chunks, IM_T), wg::blocks_for(a.pairs, a.rp));
  if (plan)
    hipLaunchKernelGGL(k_import<true>, grid, dim3(IM_T), 0, wg::as_stream(stream), a);
  else
    hipLaunchKernelGGL(k_import<false>, grid, dim3(IM_T), 0, wg::as_stream(stream), a);
  return wg::check_launch("k_import");
}
}  // namespace

extern "C" int wg_import_rgba(const uint8_t* rgba, int32_t w, int32_t h, int32_t stride, int64_t rgba_pitch,
                              int32_t has_alpha, uint8_t* y, uint8_t* u, uint8_t* v, int64_t y_pitch,
                              int64_t uv_pitch, int32_t n_images, void* stream) {
  return launch_import(rgba, w, h, stride, rgba_pitch, has_alpha, y, u, v, y_pitch, uv_pitch, n_images, 0, nullptr,
                       stream);
}

// webp.Encode's dithering strength (encode.go (root):517-521, float32) and
// InitRandom's amplitude (random.go:39-49).
extern "C" int32_t wg_dither_amp(float quality, int32_t preprocessing) {
  if (!(preprocessing & 2)) return 0;
  const float x = quality / 100.0f;
  const float x2 = x * x;
  const float dithering = 1.0f + (0.5f - 1.0f) * x2 * x2;
  if (dithering < 0.0f) return 0;
  if (dithering > 1.0f) return 1 << 8;
  return (int32_t)((float)(1 << 8) * dithering);
}

extern "C" size_t wg_dither_plan_bytes(int32_t w, int32_t h) {
  if (w <= 0 || h <= 0) return 0;
  const size_t padw = 16 * (size_t)((w + 15) >> 4), padh = 16 * (size_t)((h + 15) >> 4);
  return padw * padh * 2 + padw * (padh / 2) * 4;
}

// The VP8Random stream of one image (InitRandom + RandomBits2 before the
// amplitude, random.go:24-72) in the order importImage draws it.
extern "C" int wg_dither_plan_host(int32_t w, int32_t h, void* plan_host) {
  WG_REQUIRE(plan_host && w > 0 && h > 0);
  const int64_t padw = 16 * (int64_t)((w + 15) >> 4), padh = 16 * (int64_t)((h + 15) >> 4);
  static const uint32_t kTab[55] = {
      0x0de15230, 0x03b31886, 0x775faccb, 0x1c88626a, 0x68385c55, 0x14b3b828, 0x4a85fef8, 0x49ddb84b, 0x64fcf397,
      0x5c550289, 0x4a290000, 0x0d7ec1da, 0x5940b7ab, 0x5492577d, 0x4e19ca72, 0x38d38c69, 0x0c01ee65, 0x32a1755f,
      0x5437f652, 0x5abb2c32, 0x0faa57b1, 0x73f533e7, 0x685feeda, 0x7563cce2, 0x6e990e83, 0x4730a7ed, 0x4fc0d9c6,
      0x496b153c, 0x4f1403fa, 0x541afb0c, 0x73990b32, 0x26d7cb1c, 0x6fcc3706, 0x2cbb77d8, 0x75762f2a, 0x6425ccdd,
      0x24b35461, 0x0a7d8715, 0x220414a8, 0x141ebf67, 0x56b41583, 0x73e502e3, 0x44cab16f, 0x28264d42, 0x73baaefb,
      0x0a50ebed, 0x1d6ab6fb, 0x0d3ad40b, 0x35db3b68, 0x2b081e83, 0x77ce6b95, 0x5181e5f0, 0x78853bbc, 0x009f9494,
      0x27e5ed3c};  // kRandomTable, random.go:24-35
  uint32_t tab[55];
  memcpy(tab, kTab, sizeof(tab));
  int i1 = 0, i2 = 31;
  auto next = [&]() -> uint32_t {  // the raw 31-bit draw, RandomBits2 :55-66
    int64_t d = (int64_t)tab[i1] - (int64_t)tab[i2];
    if (d < 0) d += (int64_t)1 << 31;
    tab[i1] = (uint32_t)d;
    if (++i1 == 55) i1 = 0;
    if (++i2 == 55) i2 = 0;
    return (uint32_t)d;
  };
  int16_t* py = static_cast<int16_t*>(plan_host);
  for (int64_t k = 0; k < padw * padh; k++) py[k] = (int16_t)((int32_t)(next() << 1) >> 16);
  int32_t* puv = reinterpret_cast<int32_t*>(py + padw * padh);
  for (int64_t k = 0; k < padw * (padh / 2); k++) puv[k] = (int32_t)(next() << 1) >> 14;
  return WG_OK;
}

extern "C" int wg_dither_plan(int32_t w, int32_t h, void* plan, void* stream) {
  WG_REQUIRE(plan && w > 0 && h > 0 && (reinterpret_cast<uintptr_t>(plan) & 15) == 0);
  const size_t bytes = wg_dither_plan_bytes(w, h);
  std::vector<uint8_t> host(bytes);
  const int rc = wg_dither_plan_host(w, h, host.data());
  if (rc) return rc;
  hipStream_t s = wg::as_stream(stream);
  if (hipMemcpyAsync(plan, host.data(), bytes, hipMemcpyHostToDevice, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return wg::check_launch("wg_dither_plan copy");
  return WG_OK;
}

// ---------------------------------------------------------------------------
// importYCbCr (internal/lossy/encode.go:544-585): 4:2:0 planes someone else
// made (sharpyuv.Convert for UseSharpYUV) into the encoder's padded planes.
// The reference clamps the source index per byte (srcX = min(x, w - 1), srcY
// = min(y, h - 1), per plane); here one thread makes a 16-byte span of a
// padded row, so a wave's loads and stores are one contiguous 1 KB each.
//
// Rows walked: per image the padded Y rows [ry0, padh), then the chroma rows
// [rc0, padh / 2), a chroma row holding U's spans and then V's (so Y and
// chroma rows are about as wide, and the three planes go in one launch).
// Copy mode walks every row (ry0 = rc0 = 0).  In place (source == the padded
// planes themselves) only the margin is stored to: the rows below the image
// are walked the same way (ry0 = h, rc0 = (h + 1) / 2), and the columns right
// of it -- less than one span wide in every plane -- by the blocks past
// row_blocks, one thread per row.  Every byte read is an interior byte (column
// < w of a row < h), which no thread stores to, so in place has no ordering
// hazard.  No LDS, no scratch.
namespace {
struct YCbCrArgs {
  const uint8_t *sy, *su, *sv;
  uint8_t *y, *u, *v;
  int64_t sy_pitch, suv_pitch, y_pitch, uv_pitch;
  int sy_stride, suv_stride;
  int w, h, cw, ch;   // source plane sizes
  int padw, padh;     // padded Y plane (chroma: half of each)
  int ys, cs;         // 16-byte spans of a padded Y row / of one plane's chroma row (the last may be 8 bytes)
  int ry0, rc0;       // first row walked of Y / of the chroma planes
  int rows_img;       // rows walked per image: (padh - ry0) + (padh / 2 - rc0)
  int rows;           // n_images * rows_img
  int rp;             // rows walked per block (grid.y stays <= 65535)
  int tx_log2;        // a block is 2^tx_log2 spans wide and YC_T >> tx_log2 rows deep
  int row_blocks;     // grid.y blocks that walk rows; the ones above take the column margin (in place)
  int edges_img;      // in place: rows with a column margin per image, h (Y) + 2 * ch (U, V); else 0
  int64_t edges;      // n_images * edges_img
};

constexpr int YC_T = 256;  // threads per block: up to 256 spans = 4096 columns of a row; rows narrower than
                           // that share a block (1920 columns: 128 spans x 2 rows), so few lanes idle
constexpr int YC_RP = 8;   // minimum rows walked per thread

// 16 (or 8: NB) clamped source bytes of row `srow` (ws wide) from column x0,
// as little-endian words.  An interior span is gathered with the widest loads
// its address allows, the span holding column ws - 1 and the margin byte by
// byte (a margin span is one byte, replicated).
template <int NB>
__device__ __forceinline__ void yc_gather(const uint8_t* srow, int ws, int x0, uint32_t (&v)[4]) {
  constexpr int NW = NB / 4;
  if (x0 + NB <= ws) {
    const uint8_t* p = srow + x0;
    const uintptr_t al = reinterpret_cast<uintptr_t>(p);
    if (NB == 16 && (al & 15) == 0) {
      const uint4 q = *reinterpret_cast<const uint4*>(p);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else if ((al & 7) == 0) {
#pragma unroll
      for (int k = 0; k < NW / 2; k++) {
        const uint2 q = reinterpret_cast<const uint2*>(p)[k];
        v[2 * k] = q.x; v[2 * k + 1] = q.y;
      }
    } else if ((al & 3) == 0) {
#pragma unroll
      for (int k = 0; k < NW; k++) v[k] = reinterpret_cast<const uint32_t*>(p)[k];
    } else if ((al & 1) == 0) {
#pragma unroll
      for (int k = 0; k < NW; k++) {
        const uint32_t lo = reinterpret_cast<const uint16_t*>(p)[2 * k], hi = reinterpret_cast<const uint16_t*>(p)[2 * k + 1];
        v[k] = lo | hi << 16;
      }
    } else {
#pragma unroll
      for (int k = 0; k < NW; k++)
        v[k] = (uint32_t)p[4 * k] | (uint32_t)p[4 * k + 1] << 8 | (uint32_t)p[4 * k + 2] << 16 | (uint32_t)p[4 * k + 3] << 24;
    }
    return;
  }
  const uint32_t edge = srow[ws - 1];
  if (x0 >= ws) {
#pragma unroll
    for (int k = 0; k < NW; k++) v[k] = edge * 0x01010101u;
    return;
  }
#pragma unroll
  for (int k = 0; k < NW; k++) {
    uint32_t word = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int x = x0 + 4 * k + i;
      const uint32_t b = x < ws ? (uint32_t)srow[x] : edge;
      word |= b << (8 * i);
    }
    v[k] = word;
  }
}

// One span of one padded row.  margin_only (in place, rows of the image): an
// interior span is left alone and the span holding column ws - 1 stores its
// margin bytes only.  drow is 4-byte aligned (the destination rules).
template <int NB>
__device__ __forceinline__ void yc_span_nb(const uint8_t* srow, int ws, uint8_t* drow, int x0, bool margin_only) {
  constexpr int NW = NB / 4;
  if (margin_only && x0 + NB <= ws) return;
  uint32_t v[4] = {0, 0, 0, 0};
  yc_gather<NB>(srow, ws, x0, v);
  uint8_t* d = drow + x0;
  if (margin_only && x0 < ws) {
#pragma unroll
    for (int i = 0; i < NB; i++)
      if (x0 + i >= ws) d[i] = (uint8_t)(v[i >> 2] >> (8 * (i & 3)));
    return;
  }
  const uintptr_t al = reinterpret_cast<uintptr_t>(d);
  if (NB == 16 && (al & 15) == 0) {
    *reinterpret_cast<uint4*>(d) = make_uint4(v[0], v[1], v[2], v[3]);
  } else if ((al & 7) == 0) {
#pragma unroll
    for (int k = 0; k < NW / 2; k++) reinterpret_cast<uint2*>(d)[k] = make_uint2(v[2 * k], v[2 * k + 1]);
  } else {
#pragma unroll
    for (int k = 0; k < NW; k++) reinterpret_cast<uint32_t*>(d)[k] = v[k];
  }
}

// span c of a padded row pw bytes wide (pw a multiple of 8: the last span of
// an odd-mbw chroma row is 8 bytes)
__device__ __forceinline__ void yc_span(const uint8_t* srow, int ws, uint8_t* drow, int pw, int c, bool margin_only) {
  const int x0 = 16 * c;
  if (x0 + 16 <= pw) yc_span_nb<16>(srow, ws, drow, x0, margin_only);
  else yc_span_nb<8>(srow, ws, drow, x0, margin_only);
}

__global__ __launch_bounds__(YC_T) void k_import_ycbcr(const YCbCrArgs a) {
  const int pcw = a.padw >> 1;
  if ((int)blockIdx.y >= a.row_blocks) {
    // in place: the columns right of the image, rows of the image; item =
    // (image, plane row), the margin is inside the row's last span
    const int64_t e = ((int64_t)(blockIdx.y - a.row_blocks) * gridDim.x + blockIdx.x) * YC_T + threadIdx.x;
    if (e >= a.edges) return;
    const int img = (int)(e / a.edges_img);
    int r = (int)(e - (int64_t)img * a.edges_img);
    if (r < a.h) {
      if (a.w < a.padw) {
        uint8_t* row = a.y + img * a.y_pitch + (int64_t)r * a.padw;
        yc_span(a.sy + img * a.sy_pitch + (int64_t)r * a.sy_stride, a.w, row, a.padw, a.ys - 1, true);
      }
      return;
    }
    r -= a.h;
    if (a.cw >= pcw) return;
    const bool second = r >= a.ch;
    if (second) r -= a.ch;
    const int64_t so = img * a.suv_pitch + (int64_t)r * a.suv_stride, dof = img * a.uv_pitch + (int64_t)r * pcw;
    yc_span((second ? a.sv : a.su) + so, a.cw, (second ? a.v : a.u) + dof, pcw, a.cs - 1, true);
    return;
  }
  const int cx = (blockIdx.x << a.tx_log2) + (threadIdx.x & ((1 << a.tx_log2) - 1));
  const int yrows = a.padh - a.ry0;
  const int row_end = min((int)(blockIdx.y + 1) * a.rp, a.rows);
  for (int rr = blockIdx.y * a.rp + (threadIdx.x >> a.tx_log2); rr < row_end; rr += YC_T >> a.tx_log2) {
    const int img = rr / a.rows_img, ri = rr - img * a.rows_img;
    if (ri < yrows) {
      if (cx >= a.ys) continue;
      const int r = a.ry0 + ri;
      yc_span(a.sy + img * a.sy_pitch + (int64_t)min(r, a.h - 1) * a.sy_stride, a.w,
              a.y + img * a.y_pitch + (int64_t)r * a.padw, a.padw, cx, false);
    } else {
      if (cx >= 2 * a.cs) continue;
      const int r = a.rc0 + ri - yrows;
      const bool second = cx >= a.cs;
      const int64_t so = img * a.suv_pitch + (int64_t)min(r, a.ch - 1) * a.suv_stride, dof = img * a.uv_pitch + (int64_t)r * pcw;
      yc_span((second ? a.sv : a.su) + so, a.cw, (second ? a.v : a.u) + dof, pcw, second ? cx - a.cs : cx, false);
    }
  }
}

// [p, p + n) and [q, q + m) share a byte
bool yc_overlap(const uint8_t* p, int64_t n, const uint8_t* q, int64_t m) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return a < b + (uintptr_t)m && b < a + (uintptr_t)n;
}
}  // namespace

extern "C" int wg_import_ycbcr(const uint8_t* sy, int32_t sy_stride, int64_t sy_pitch, const uint8_t* su,
                               const uint8_t* sv, int32_t suv_stride, int64_t suv_pitch, int32_t w, int32_t h,
                               uint8_t* y, uint8_t* u, uint8_t* v, int64_t y_pitch, int64_t uv_pitch, int32_t n_images,
                               void* stream) {
  WG_REQUIRE(sy && su && sv && y && u && v);
  WG_REQUIRE(w > 0 && h > 0 && n_images > 0);
  const int cw = (w + 1) >> 1, ch = (h + 1) >> 1;
  const int mbw = (w + 15) >> 4, mbh = (h + 15) >> 4;
  const int64_t ybytes = (int64_t)256 * mbw * mbh, cbytes = (int64_t)64 * mbw * mbh;
  const int64_t sy_bytes = (int64_t)(h - 1) * sy_stride + w, sc_bytes = (int64_t)(ch - 1) * suv_stride + cw;
  WG_REQUIRE(sy_stride >= w && suv_stride >= cw && sy_pitch >= sy_bytes && suv_pitch >= sc_bytes);
  WG_REQUIRE(((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(u) | reinterpret_cast<uintptr_t>(v)) &
              3) == 0 && (y_pitch & 7) == 0 && (uv_pitch & 3) == 0);
  WG_REQUIRE(y_pitch >= ybytes && uv_pitch >= cbytes);
  const bool in_place = sy == y && su == u && sv == v && sy_stride == 16 * mbw && suv_stride == 8 * mbw &&
                        sy_pitch == y_pitch && suv_pitch == uv_pitch;
  if (!in_place) {
    // the byte ranges the n images of a source plane and of a destination
    // plane span must be disjoint
    const int64_t last = n_images - 1;
    const uint8_t* src[3] = {sy, su, sv};
    const int64_t src_n[3] = {last * sy_pitch + sy_bytes, last * suv_pitch + sc_bytes, last * suv_pitch + sc_bytes};
    const uint8_t* dst[3] = {y, u, v};
    const int64_t dst_n[3] = {last * y_pitch + ybytes, last * uv_pitch + cbytes, last * uv_pitch + cbytes};
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++)
        if (yc_overlap(src[i], src_n[i], dst[j], dst_n[j]))
          return wg::invalid("wg_import_ycbcr: source and destination overlap (in place needs the same pointers, "
                             "strides 16*mbw / 8*mbw and the same pitches)");
  }
  YCbCrArgs a;
  a.sy = sy;
  a.su = su;
  a.sv = sv;
  a.y = y;
  a.u = u;
  a.v = v;
  a.sy_pitch = sy_pitch;
  a.suv_pitch = suv_pitch;
  a.y_pitch = y_pitch;
  a.uv_pitch = uv_pitch;
  a.sy_stride = sy_stride;
  a.suv_stride = suv_stride;
  a.w = w;
  a.h = h;
  a.cw = cw;
  a.ch = ch;
  a.padw = 16 * mbw;
  a.padh = 16 * mbh;
  a.ys = mbw;
  a.cs = (mbw + 1) >> 1;
  a.ry0 = in_place ? h : 0;
  a.rc0 = in_place ? ch : 0;
  a.rows_img = (a.padh - a.ry0) + (a.padh / 2 - a.rc0);
  WG_REQUIRE((int64_t)n_images * a.rows_img < (1ll << 31) / 2);
  a.rows = n_images * a.rows_img;
  const int spans = max(a.ys, 2 * a.cs);
  a.tx_log2 = 0;
  while ((1 << a.tx_log2) < min(spans, YC_T)) a.tx_log2++;
  const unsigned gx = wg::blocks_for(spans, 1 << a.tx_log2);
  a.rp = max(YC_RP * (YC_T >> a.tx_log2), (int)wg::blocks_for(a.rows, 65535 / 2));
  a.row_blocks = (int)wg::blocks_for(a.rows, a.rp);
  // (the chroma margin is empty whenever the luma one is: w = 16 * mbw)
  a.edges_img = in_place && w < a.padw ? h + 2 * ch : 0;
  a.edges = (int64_t)n_images * a.edges_img;
  const int64_t edge_blocks = (a.edges + (int64_t)gx * YC_T - 1) / ((int64_t)gx * YC_T);
  WG_REQUIRE(edge_blocks <= 65535 / 2);
  if (a.row_blocks + edge_blocks == 0) return WG_OK;  // in place, no margin
  const dim3 grid(gx, (unsigned)(a.row_blocks + edge_blocks));
  hipLaunchKernelGGL(k_import_ycbcr, grid, dim3(YC_T), 0, wg::as_stream(stream), a);
  return wg::check_launch("k_import_ycbcr");
}

extern "C" int wg_import_rgba_dithered(const uint8_t* rgba, int32_t w, int32_t h, int32_t stride, int64_t rgba_pitch,
                                       int32_t has_alpha, int32_t amp, const void* plan, uint8_t* y, uint8_t* u,
                                       uint8_t* v, int64_t y_pitch, int64_t uv_pitch, int32_t n_images,
                                       void* stream) {
  WG_REQUIRE(plan && (reinterpret_cast<uintptr_t>(plan) & 15) == 0 && amp >= 0 && amp <= 256);
  return launch_import(rgba, w, h, stride, rgba_pitch, has_alpha, y, u, v, y_pitch, uv_pitch, n_images, amp, plan,
                       stream);
}
