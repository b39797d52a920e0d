// vp8_emit_main.cpp -- stand-alone driver of webp_amd/csrc/vp8_emit.cpp for a
// sanitizer build (tests/test_phase_b.py compiles both with g++
// -fsanitize=address,undefined and runs the binary; no HIP, no Python).
// Input file: per case eight int32 (width, height, mbw, mbh, log2_parts, riff,
// token bytes, expected file bytes), then wg_enc_config, wg_frame_segs,
// wg_mb_hdr[mbw*mbh], 1056 probabilities, wg_token_summary, the token bytes
// and the expected file.  Every array is copied into an exactly sized heap
// block so that a read past its end is caught.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../include/webpgpu.h"

namespace wg {
static std::string g_error;
void set_error(const std::string& msg) { g_error = msg; }
}  // namespace wg

static bool read_exact(FILE* f, std::vector<uint8_t>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), 1, n, f) == n;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int cases = 0;
  int32_t h[8];
  while (fread(h, sizeof(int32_t), 8, f) == 8) {
    const size_t nmb = (size_t)h[2] * (size_t)h[3];
    std::vector<uint8_t> cfg, info, hdr, proba, summary, tokens, expect;
    if (!read_exact(f, cfg, sizeof(wg_enc_config)) || !read_exact(f, info, sizeof(wg_frame_segs)) ||
        !read_exact(f, hdr, nmb * sizeof(wg_mb_hdr)) || !read_exact(f, proba, 1056) ||
        !read_exact(f, summary, sizeof(wg_token_summary)) || !read_exact(f, tokens, (size_t)h[6]) ||
        !read_exact(f, expect, (size_t)h[7])) {
      fprintf(stderr, "case %d: truncated input\n", cases);
      return 1;
    }
    wg_enc_config c;
    wg_frame_segs fs;
    wg_token_summary ts;
    memcpy(&c, cfg.data(), sizeof(c));
    memcpy(&fs, info.data(), sizeof(fs));
    memcpy(&ts, summary.data(), sizeof(ts));
    std::vector<wg_mb_hdr> hd(nmb);
    memcpy(hd.data(), hdr.data(), hdr.size());
    const size_t bound = wg_vp8_emit_bound(h[2], h[3], ts.total_tokens);
    // first the exact size through WG_ENOMEM, then an exactly sized buffer
    size_t size = 0;
    int rc = wg_vp8_emit(h[0], h[1], h[2], h[3], &c, &fs, hd.data(), proba.data(), &ts, tokens.data(), h[4], h[5],
                         nullptr, 0, &size);
    if (rc != WG_ENOMEM || size != expect.size() || size > bound) {
      fprintf(stderr, "case %d: size query gave %d, %zu (expected %zu, bound %zu)\n", cases, rc, size, expect.size(), bound);
      return 1;
    }
    std::vector<uint8_t> out(size);
    rc = wg_vp8_emit(h[0], h[1], h[2], h[3], &c, &fs, hd.data(), proba.data(), &ts, tokens.data(), h[4], h[5],
                     out.data(), out.size(), &size);
    if (rc != WG_OK || size != expect.size() || memcmp(out.data(), expect.data(), size) != 0) {
      fprintf(stderr, "case %d: emit gave %d (%s), %zu bytes\n", cases, rc, wg::g_error.c_str(), size);
      return 1;
    }
    cases++;
  }
  fclose(f);
  printf("vp8_emit_main: %d cases ok\n", cases);
  return 0;
}
