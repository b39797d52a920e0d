// vp8_emit.cpp -- host-side VP8 (lossy) bitstream writer: the encoder's
// counterpart of vp8_parse.cpp.  Takes what wg_encode_token_stats /
// wg_encode_tokens leave per image (wg_mb_hdr, the probabilities, the
// {bit, prob} token pairs) plus the frame's header record and writes the file.
//
// Follows, in order:
//   boolean encoder               internal/bitio/writer_bool.go:1-258
//   partition 0                   internal/lossy/encode_syntax.go:47-102 (emitPartition0)
//   segment / filter / quantiser  encode_syntax.go:175-322, encode_analysis.go:852-868
//                                 (buildSegmentHeader), encode.go:1276-1319 (setupFilterStrength)
//   token probabilities           encode_syntax.go:325-344 (writeCoeffProba)
//   intra modes                   encode_syntax.go:349-500 (writeMBModes and the mode trees)
//   token partitions              encode_syntax.go:105-114, encode_token.go:304-361
//   frame assembly, container     encode_syntax.go:118-172 (assembleFrame), :511-538 (AssembleRIFF)
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/webpgpu.h"
#include "vp8_tables.h"
#include "wg_common_host.h"

namespace {

// 8 - floor(log2(range + 1)) for range in [0, 127] (kNorm, writer_bool.go:237)
inline int norm_shift(int32_t range) { return 7 ^ (31 - __builtin_clz((uint32_t)range + 1)); }

// BoolWriter (writer_bool.go): VP8BitWriter's arithmetic.
struct BoolWriter {
  int32_t range = 255 - 1, value = 0;
  int run = 0, nb_bits = -8;
  std::vector<uint8_t> buf;

  void renorm() {
    if (range < 127) {
      const int shift = norm_shift(range);
      range = ((range + 1) << shift) - 1;  // kNewRange
      value <<= shift;
      nb_bits += shift;
      if (nb_bits > 0) flush();
    }
  }
  void put(int bit, int prob) {  // PutBit :58-76
    const int32_t split = (range * prob) >> 8;
    if (bit) {
      value += split + 1;
      range -= split + 1;
    } else {
      range = split;
    }
    renorm();
  }
  void put_uniform(int bit) {  // PutBitUniform :80-97
    const int32_t split = range >> 1;
    if (bit) {
      value += split + 1;
      range -= split + 1;
    } else {
      range = split;
    }
    renorm();  // range in [63, 126] here: the shift is 1, as written there
  }
  void put_bits(uint32_t v, int n) {  // PutBits :148-156
    for (uint32_t mask = n > 0 ? 1u << (n - 1) : 0; mask; mask >>= 1) put_uniform((v & mask) != 0);
  }
  void put_signed(int v, int n) {  // PutSignedBits :161-170
    put_uniform(v != 0);
    if (v == 0) return;
    if (v < 0) put_bits(((uint32_t)-v << 1) | 1, n + 1);
    else put_bits((uint32_t)v << 1, n + 1);
  }
  void put_packed(const uint8_t* data, size_t count) {  // PutBitBatchPacked :106-144
    for (size_t i = 0; i < count; i++) put(data[2 * i], data[2 * i + 1]);
  }
  void flush() {  // :174-201
    const int s = 8 + nb_bits;
    const int32_t bits = value >> s;
    value -= bits << s;
    nb_bits -= 8;
    if ((bits & 0xff) != 0xff) {
      if ((bits & 0x100) && !buf.empty()) buf.back()++;
      if (run > 0) {
        buf.insert(buf.end(), (size_t)run, (bits & 0x100) ? 0x00 : 0xff);
        run = 0;
      }
      buf.push_back((uint8_t)(bits & 0xff));
    } else {
      run++;
    }
  }
  void finish() {  // :205-210
    put_bits(0, 9 - nb_bits);
    nb_bits = 0;
    flush();
  }
};

int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// buildSegmentHeader (encode_analysis.go:852-868) + writeSegmentHeader (encode_syntax.go:175-235)
void write_segment_header(BoolWriter& bw, const wg_enc_config* cfg, const wg_frame_segs* info, bool use_segment,
                          bool update_map) {
  bw.put_uniform(use_segment);
  if (!use_segment) return;
  bw.put_uniform(update_map);
  bw.put_uniform(1);  // update segment data
  bw.put_uniform(1);  // AbsoluteDelta
  const int nseg = clampi(info->num_segments, 0, 4);
  int quant[4] = {0, 0, 0, 0}, fstr[4] = {0, 0, 0, 0};
  const int qstep0 = vp8_ac_table[clampi(info->quant[0], 0, 127)] >> 2;
  for (int i = 0; i < nseg; i++) {
    quant[i] = (int8_t)clampi(info->quant[i], -127, 127);
    const int qstep = vp8_ac_table[clampi(info->quant[i], 0, 127)] >> 2;
    fstr[i] = clampi((qstep - qstep0) * cfg->filter_strength / 100, -63, 63);
  }
  for (int i = 0; i < 4; i++) {
    bw.put_uniform(quant[i] != 0);
    if (quant[i]) {
      bw.put_bits((uint32_t)(quant[i] < 0 ? -quant[i] : quant[i]), 7);
      bw.put_uniform(quant[i] < 0);
    }
  }
  for (int i = 0; i < 4; i++) {
    bw.put_uniform(fstr[i] != 0);
    if (fstr[i]) {
      bw.put_bits((uint32_t)(fstr[i] < 0 ? -fstr[i] : fstr[i]), 6);
      bw.put_uniform(fstr[i] < 0);
    }
  }
  if (update_map)
    for (int i = 0; i < 3; i++) {
      bw.put_uniform(info->seg_proba[i] != 255);
      if (info->seg_proba[i] != 255) bw.put_bits(info->seg_proba[i], 8);
    }
}

// i4SubtreeContains (encode_syntax.go:474-480)
bool subtree_contains(int node, int mode) {
  if (node <= 0) return -node == mode;
  return subtree_contains(vp8_ymodes_intra4[2 * node], mode) || subtree_contains(vp8_ymodes_intra4[2 * node + 1], mode);
}

// writeI4ModeBits (encode_syntax.go:445-469)
void write_i4_mode(BoolWriter& bw, int mode, const uint8_t* prob) {
  int bit = !subtree_contains(vp8_ymodes_intra4[0], mode);
  bw.put(bit, prob[0]);
  int i = vp8_ymodes_intra4[bit];
  while (i > 0) {
    bit = !subtree_contains(vp8_ymodes_intra4[2 * i], mode);
    bw.put(bit, prob[i]);
    i = vp8_ymodes_intra4[2 * i + bit];
  }
}

// writeMBModes (encode_syntax.go:349-410) with writeSegmentID :413, writeI16Mode :425, writeUVMode :484
void write_mb_modes(BoolWriter& bw, const wg_mb_hdr* hdr, int mbw, int mbh, bool write_segment,
                    const uint8_t* seg_proba, bool use_skip, int skip_proba) {
  std::vector<uint8_t> top_modes(4 * (size_t)mbw, 0);
  for (int y = 0; y < mbh; y++) {
    uint8_t left[4] = {0, 0, 0, 0};
    for (int x = 0; x < mbw; x++) {
      const wg_mb_hdr& h = hdr[(size_t)y * mbw + x];
      uint8_t* top = &top_modes[4 * (size_t)x];
      if (write_segment) {
        const int id = h.segment & 3;
        bw.put((id >> 1) & 1, seg_proba[0]);
        bw.put(id & 1, id >= 2 ? seg_proba[2] : seg_proba[1]);
      }
      if (use_skip) bw.put(h.skip != 0, skip_proba);
      if (h.mb_type == 0) {
        bw.put(1, 145);
        const int m = h.i16_mode & 3;  // DC 0, TM 1, V 2, H 3 (constants.go)
        if (m == 1 || m == 3) {
          bw.put(1, 156);
          bw.put(m == 1, 128);
        } else {
          bw.put(0, 156);
          bw.put(m == 2, 163);
        }
        memset(top, h.i16_mode, 4);
        memset(left, h.i16_mode, 4);
      } else {
        bw.put(0, 145);
        for (int by = 0; by < 4; by++) {
          int ymode = left[by];
          for (int bx = 0; bx < 4; bx++) {
            const int mode = h.modes[by * 4 + bx];
            write_i4_mode(bw, mode, vp8_bmodes_proba + (top[bx] * 10 + ymode) * 9);
            ymode = mode;
            top[bx] = (uint8_t)mode;
          }
          left[by] = (uint8_t)ymode;
        }
      }
      const int uv = h.uv_mode & 3;
      if (uv == 0) {
        bw.put(0, 142);
      } else if (uv == 2) {
        bw.put(1, 142);
        bw.put(0, 114);
      } else {
        bw.put(1, 142);
        bw.put(1, 114);
        bw.put(uv == 1, 183);
      }
    }
  }
}

constexpr size_t kHeaderSymbols = 2 + 99 + 11 + 2 + 37 + 1 + 1056 * 9 + 9;  // everything of partition 0 before the modes
constexpr size_t kMbModeSymbols = 2 + 1 + 1 + 16 * 9 + 3;  // segment id, skip, type, 16 I4 modes (tree depth <= 9), chroma mode

}  // namespace

// Upper bound of wg_vp8_emit's output.  The bool writer renormalises by at
// most 7 bits a symbol when the symbol's probability is at least 1/256 (a
// range below 127 is shifted up by kNorm <= 7), so every bool-coded symbol
// costs at most one byte; Finish adds at most 2 bytes and each pending run of
// 0xff bytes was already counted by the symbols that made it.  Partition 0
// has at most kHeaderSymbols + kMbModeSymbols per MB symbols, the token
// partitions total_tokens; 10 bytes of frame tag and picture header, 3 per
// extra partition size, 20 of RIFF + chunk header, 1 of padding.
extern "C" size_t wg_vp8_emit_bound(int32_t mbw, int32_t mbh, uint32_t total_tokens) {
  if (mbw <= 0 || mbh <= 0) return 0;
  const size_t nmb = (size_t)mbw * (size_t)mbh;
  return 10 + kHeaderSymbols + kMbModeSymbols * nmb + 4 + (size_t)total_tokens + 8 * 4 + 3 * 7 + 20 + 1;
}

extern "C" int wg_vp8_emit(int32_t width, int32_t height, int32_t mbw, int32_t mbh, const wg_enc_config* cfg,
                           const wg_frame_segs* info,
                           const wg_mb_hdr* hdr, const uint8_t* proba, const wg_token_summary* summary,
                           const uint8_t* tokens, int32_t log2_parts, int32_t riff, uint8_t* out, size_t out_cap,
                           size_t* out_size) {
  WG_REQUIRE(cfg && info && hdr && proba && summary && out_size);
  WG_REQUIRE(out || out_cap == 0);
  WG_REQUIRE(tokens || summary->total_tokens == 0);
  WG_REQUIRE(width > 0 && height > 0 && width <= 0x3fff && height <= 0x3fff);
  WG_REQUIRE(log2_parts >= 0 && log2_parts <= 3);
  // the MB grid the records were made for must be this picture's
  WG_REQUIRE(mbw == (width + 15) >> 4 && mbh == (height + 15) >> 4);
  const size_t nmb = (size_t)mbw * mbh;
  uint64_t last_end = 0;
  for (size_t i = 0; i < nmb; i++) {
    if (hdr[i].i16_mode > 3 || hdr[i].uv_mode > 3) return wg::invalid("hdr: prediction mode out of range");
    if (hdr[i].mb_type != 0)
      for (int k = 0; k < 16; k++)
        if (hdr[i].modes[k] > 9) return wg::invalid("hdr: I4 mode out of range");
    const uint64_t end = (uint64_t)hdr[i].tok_start + hdr[i].tok_count;
    if (end > summary->total_tokens) return wg::invalid("hdr token ranges pass summary->total_tokens (hdr and summary of different images?)");
    if (end > last_end) last_end = end;
  }
  if (last_end != summary->total_tokens) return wg::invalid("hdr token ranges do not cover summary->total_tokens (hdr and summary of different images?)");

  // ---- partition 0 (emitPartition0)
  BoolWriter p0;
  p0.buf.reserve(nmb * 8 + 1024);
  p0.put_uniform(0);  // colorspace
  p0.put_uniform(0);  // clamp type
  const bool use_segment = info->num_segments > 1;
  const bool update_map = use_segment && info->update_map != 0;
  write_segment_header(p0, cfg, info, use_segment, update_map);
  // writeFilterHeader: UseLFDelta is never set (encode.go:1283-1285)
  p0.put_uniform(cfg->filter_type == 0);
  p0.put_bits((uint32_t)clampi(info->filter_level, 0, 63), 6);
  p0.put_bits((uint32_t)clampi(cfg->filter_sharpness, 0, 7), 3);
  p0.put_uniform(0);
  p0.put_bits((uint32_t)log2_parts, 2);
  // writeQuantParams: dq y1_dc, y2_dc, y2_ac are 0
  p0.put_bits((uint32_t)clampi(info->base_quant, 0, 127), 7);
  p0.put_signed(0, 4);
  p0.put_signed(0, 4);
  p0.put_signed(0, 4);
  p0.put_signed(info->dq_uv_dc, 4);
  p0.put_signed(info->dq_uv_ac, 4);
  p0.put_uniform(0);  // refresh-update flag
  for (int k = 0; k < 1056; k++) {  // writeCoeffProba
    if (proba[k] != vp8_coeffs_proba0[k]) {
      p0.put(1, vp8_coeffs_update_proba[k]);
      p0.put_bits(proba[k], 8);
    } else {
      p0.put(0, vp8_coeffs_update_proba[k]);
    }
  }
  const bool use_skip = summary->num_skip > 0;
  p0.put_uniform(use_skip);
  if (use_skip) p0.put_bits(summary->skip_proba, 8);
  write_mb_modes(p0, hdr, mbw, mbh, update_map, info->seg_proba, use_skip, summary->skip_proba);
  p0.finish();

  // ---- token partitions (emitTokenPartitions, EmitTokensPartitioned)
  const int nparts = 1 << log2_parts;
  std::vector<BoolWriter> parts((size_t)nparts);
  for (int p = 0; p < nparts; p++) parts[(size_t)p].buf.reserve((size_t)summary->total_tokens / (2 * nparts) + 64);
  for (int y = 0; y < mbh; y++) {
    BoolWriter& bw = parts[(size_t)(y & (nparts - 1))];
    for (int x = 0; x < mbw; x++) {
      const wg_mb_hdr& h = hdr[(size_t)y * mbw + x];
      bw.put_packed(tokens + 2 * (size_t)h.tok_start, h.tok_count);
    }
  }
  for (int p = 0; p < nparts; p++) parts[(size_t)p].finish();

  // ---- assembleFrame + AssembleRIFF
  if (p0.buf.size() >= (1u << 19)) return wg::invalid("partition 0 does not fit the frame tag's 19 bits");
  size_t vp8_size = 10 + p0.buf.size() + 3 * (size_t)(nparts - 1);
  for (int p = 0; p < nparts; p++) {
    if (p < nparts - 1 && parts[(size_t)p].buf.size() >= (1u << 24)) return wg::invalid("a token partition does not fit its 24-bit size");
    vp8_size += parts[(size_t)p].buf.size();
  }
  const size_t total = riff ? 20 + vp8_size + (vp8_size & 1) : vp8_size;
  *out_size = total;
  if (total > out_cap) {
    wg::set_error("wg_vp8_emit: out_cap is smaller than the file");
    return WG_ENOMEM;
  }
  uint8_t* o = out;
  auto put32 = [&](uint32_t v) {
    for (int k = 0; k < 4; k++) *o++ = (uint8_t)(v >> (8 * k));
  };
  if (riff) {
    memcpy(o, "RIFF", 4);
    o += 4;
    put32((uint32_t)(12 + vp8_size + (vp8_size & 1)));
    memcpy(o, "WEBPVP8 ", 8);
    o += 8;
    put32((uint32_t)vp8_size);
  }
  const uint32_t tag = (1u << 4) | ((uint32_t)p0.buf.size() << 5);  // key frame, profile 0, show
  *o++ = (uint8_t)tag;
  *o++ = (uint8_t)(tag >> 8);
  *o++ = (uint8_t)(tag >> 16);
  *o++ = 0x9d;
  *o++ = 0x01;
  *o++ = 0x2a;
  *o++ = (uint8_t)(width & 0xff);
  *o++ = (uint8_t)((width >> 8) & 0x3f);
  *o++ = (uint8_t)(height & 0xff);
  *o++ = (uint8_t)((height >> 8) & 0x3f);
  memcpy(o, p0.buf.data(), p0.buf.size());
  o += p0.buf.size();
  for (int p = 0; p + 1 < nparts; p++) {
    const size_t sz = parts[(size_t)p].buf.size();
    *o++ = (uint8_t)sz;
    *o++ = (uint8_t)(sz >> 8);
    *o++ = (uint8_t)(sz >> 16);
  }
  for (int p = 0; p < nparts; p++) {
    const std::vector<uint8_t>& b = parts[(size_t)p].buf;
    if (!b.empty()) memcpy(o, b.data(), b.size());
    o += b.size();
  }
  if (riff && (vp8_size & 1)) *o++ = 0;
  return WG_OK;
}
