// multi_device.hip -- the multi-device batch variant of the encode DSP path
// (last bullet; 8(e) C4) for a host that drives every GPU from
// one process, as the reference's Go program would through cgo.
//
// Frame i belongs to device devices[i % n_devices] (round-robin, the ownership
// webp_amd/shard.py frames_of uses for the one-process-per-GPU path).  Each
// device runs the whole device encode path over its frames on a stream of
// its own -- import (importImage, internal/lossy/encode.go:671-943) ->
// computeAlphas (encode_analysis.go:245-307) -> analysis() segments
// (encode_analysis.go:29-903) -> Phase A of encodeFrameParallel
// (encode_parallel.go:168-232) -- with no exchange between devices.  The only
// cross-device step is the final gather: every frame's MBEncInfo records,
// reconstruction, segment map and segment header come back to the caller's
// host buffers in frame order, which is where the reference's Phase B
// (recordAllTokens, encode_parallel.go:1497) and the bitstream writer run.
#include <algorithm>
#include <map>
#include <mutex>
#include <vector>

#include "vp8_tables.h"
#include "wg_common.h"

namespace {

inline size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

// the status of a HIP call (named `what` in the error)
int hip_rc(hipError_t e, const char* what) {
  if (e != hipSuccess) wg::set_error(std::string(what) + ": " + hipGetErrorString(e));
  return e == hipSuccess ? WG_OK : WG_EHIP;
}

// The caller's host buffers, page-locked for the duration of the call
// (hipHostRegister, portable to every device), so the per-device uploads and
// the gather are DMA transfers that overlap across devices instead of
// copies staged through the runtime's bounce buffers.
//
// Registrations are reference-counted across the process: concurrent calls
// (host threads) may pass the same or overlapping host buffers, and a range
// is unregistered only when the last call holding it returns -- never under
// another call's in-flight DMA.  A range that lies inside one this library
// registered takes a reference on it; one that cannot be registered (pinned
// by the caller, or overlapping a registered range) holds references on every
// registered range it overlaps and is copied as it is.
struct PinRange {
  size_t n;
  int refs;
};
std::mutex g_pin_mu;
std::map<uintptr_t, PinRange> g_pins;  // by start address

struct HostPins {
  std::vector<uintptr_t> held;  // starts of the g_pins ranges this call holds a reference on
  void pin(const void* p, size_t n) {
    if (!p || n == 0) return;
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), e = a + n;
    std::lock_guard<std::mutex> lock(g_pin_mu);
    // registered ranges overlapping [a, e)
    std::vector<uintptr_t> over;
    auto it = g_pins.upper_bound(a);
    if (it != g_pins.begin()) --it;
    for (; it != g_pins.end() && it->first < e; ++it)
      if (it->first + it->second.n > a) over.push_back(it->first);
    if (over.empty() && hipHostRegister(const_cast<void*>(p), n, hipHostRegisterPortable) == hipSuccess) {
      g_pins[a] = PinRange{n, 1};
      held.push_back(a);
      return;
    }
    (void)hipGetLastError();  // not fatal: the copies stay correct
    for (uintptr_t k : over) {
      g_pins[k].refs++;
      held.push_back(k);
    }
  }
  ~HostPins() {
    std::lock_guard<std::mutex> lock(g_pin_mu);
    for (uintptr_t k : held) {
      auto it = g_pins.find(k);
      if (it == g_pins.end()) continue;
      if (--it->second.refs == 0) {
        (void)hipHostUnregister(reinterpret_cast<void*>(k));
        g_pins.erase(it);
      }
    }
  }
};

// A first kernel on a new stream (its hardware queue is created then), issued
// before any persistent kernel runs: creating a queue while wg_encode_mbs runs
// on another one stalled it past its dependency-wait bound (webpgpu.h).
hipError_t bind_stream(void* mem, hipStream_t s) {
  hipError_t e = hipMemsetAsync(mem, 0, 256, s);
  return e == hipSuccess ? hipStreamSynchronize(s) : e;
}

// Restores the caller's current device on every return path.
struct DeviceGuard {
  int prev = -1;
  hipError_t save() { return hipGetDevice(&prev); }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// One device's share of a call: a stream of its own and one allocation,
// carved in order; released when it goes, once the stream has drained.
struct Lane {
  int dev = 0;
  hipStream_t stream = nullptr;
  void* mem = nullptr;
  size_t used = 0;
  Lane() = default;
  Lane(const Lane&) = delete;
  Lane& operator=(const Lane&) = delete;
  ~Lane() {
    if (!stream && !mem) return;
    (void)hipSetDevice(dev);
    if (stream) (void)hipStreamSynchronize(stream);
    if (mem) (void)hipFree(mem);
    if (stream) (void)hipStreamDestroy(stream);
  }
  // the next `bytes` of the allocation, 256-byte aligned
  template <class T>
  T* take(size_t bytes) {
    T* p = mem ? reinterpret_cast<T*>(static_cast<uint8_t*>(mem) + used) : nullptr;
    used += align_up(bytes);
    return p;
  }
  // Makes `device` current and creates the lane's stream and allocation:
  // `layout` (the lane's take() calls) runs once to size it, then to carve it.
  template <class F>
  hipError_t open(int device, F&& layout) {
    dev = device;
    hipError_t e = hipSetDevice(dev);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
    layout();
    if (e == hipSuccess) e = hipMalloc(&mem, used);
    used = 0;
    if (e == hipSuccess) layout();
    return e;
  }
};

// One step of a call on every open lane in turn, the lane's device current:
// rc = fn(lane), until one fails (nothing at all once rc is an error).
template <class L, class F>
int each_lane(std::vector<L>& lanes, int rc, F&& fn) {
  for (auto& l : lanes)
    if (l.mem && rc == WG_OK && (rc = hip_rc(hipSetDevice(l.dev), "hipSetDevice")) == WG_OK) rc = fn(l);
  return rc;
}
// Every lane's gather is in flight: now wait for each.
template <class L>
int wait_lanes(std::vector<L>& lanes, int rc, const char* what) {
  return each_lane(lanes, rc, [&](L& l) { return hip_rc(hipStreamSynchronize(l.stream), what); });
}

// a device may appear more than once: each entry gets its own lane (how the
// tests split work on a one-GPU box)
int check_devices(const int32_t* devices, int32_t n_devices) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess) return wg::check_launch("hipGetDeviceCount");
  for (int k = 0; k < n_devices; k++) WG_REQUIRE(devices[k] >= 0 && devices[k] < count);
  return WG_OK;
}

struct EncLane : Lane {
  std::vector<int> frames;  // global frame indices, in order
  uint8_t *rgba, *y, *u, *v, *seg_ids, *segs, *proba, *out, *work, *ry, *ru, *rv;
  int32_t *alphas, *uv_sum;
  wg_frame_segs* info;
};

}  // namespace

extern "C" int wg_encode_frames_devices(const int32_t* devices, int32_t n_devices, const uint8_t* rgba, int32_t w,
                                        int32_t h, int32_t n_images, int32_t has_alpha, const wg_enc_config* cfg,
                                        void* mb_out, uint8_t* ry, uint8_t* ru, uint8_t* rv, uint8_t* seg_ids_out,
                                        wg_frame_segs* info_out) {
  WG_REQUIRE(devices && n_devices > 0 && rgba && cfg && mb_out);
  WG_REQUIRE(w > 0 && h > 0 && n_images > 0);
  if (int rc = check_devices(devices, n_devices)) return rc;
  const int mbw = (w + 15) >> 4, mbh = (h + 15) >> 4;
  if (mbh < 4) return wg::invalid("mbh >= 4 (encode.go:1356 encodes smaller frames serially)");
  const int64_t n_mb = (int64_t)mbw * mbh, rec_b = n_mb * (int64_t)sizeof(wg_mb_enc);
  const int64_t rgba_b = (int64_t)w * h * 4, y_b = 256 * n_mb, uv_b = 64 * n_mb, seg_pitch = 4 * sizeof(wg_segment);
  DeviceGuard guard;
  if (guard.save() != hipSuccess) return wg::check_launch("hipGetDevice");
  HostPins pins;
  pins.pin(rgba, (size_t)(rgba_b * n_images));
  pins.pin(mb_out, (size_t)(rec_b * n_images));
  pins.pin(ry, (size_t)(y_b * n_images));
  pins.pin(ru, (size_t)(uv_b * n_images));
  pins.pin(rv, (size_t)(uv_b * n_images));
  pins.pin(seg_ids_out, (size_t)(n_mb * n_images));
  pins.pin(info_out, (size_t)n_images * sizeof(wg_frame_segs));

  std::vector<EncLane> jobs((size_t)n_devices);
  for (int i = 0; i < n_images; i++) jobs[(size_t)(i % n_devices)].frames.push_back(i);
  int rc = WG_OK;
  // every device's stream and buffers first (the streams bound to their
  // queues before any persistent kernel runs), then every device's work, so
  // the devices run at once
  for (auto& j : jobs) {
    const int nk = (int)j.frames.size();
    if (nk == 0) continue;
    hipError_t e = j.open(devices[&j - jobs.data()], [&] {
      j.rgba = j.take<uint8_t>((size_t)(rgba_b * nk));
      j.y = j.take<uint8_t>((size_t)(y_b * nk));
      j.u = j.take<uint8_t>((size_t)(uv_b * nk));
      j.v = j.take<uint8_t>((size_t)(uv_b * nk));
      j.seg_ids = j.take<uint8_t>((size_t)(n_mb * nk));
      j.segs = j.take<uint8_t>((size_t)(seg_pitch * nk));
      j.proba = j.take<uint8_t>(sizeof(vp8_coeffs_proba0));
      j.out = j.take<uint8_t>((size_t)(rec_b * nk));
      j.work = j.take<uint8_t>(wg_encode_work_bytes(mbw, mbh, nk));
      j.ry = j.take<uint8_t>((size_t)(y_b * nk));
      j.ru = j.take<uint8_t>((size_t)(uv_b * nk));
      j.rv = j.take<uint8_t>((size_t)(uv_b * nk));
      j.alphas = j.take<int32_t>((size_t)(n_mb * nk) * 4);
      j.uv_sum = j.take<int32_t>((size_t)nk * 4);
      j.info = j.take<wg_frame_segs>((size_t)nk * sizeof(wg_frame_segs));
    });
    if (e == hipSuccess) e = bind_stream(j.mem, j.stream);
    if ((rc = hip_rc(e, "device setup (encode batch)")) != WG_OK) break;
  }
  rc = each_lane(jobs, rc, [&](EncLane& j) {
    const int nk = (int)j.frames.size();
    void* st = j.stream;
    hipError_t e = hipSuccess;
    for (int q = 0; q < nk && e == hipSuccess; q++)
      e = hipMemcpyAsync(j.rgba + q * rgba_b, rgba + (int64_t)j.frames[(size_t)q] * rgba_b, (size_t)rgba_b,
                         hipMemcpyHostToDevice, j.stream);
    if (e == hipSuccess)
      e = hipMemcpyAsync(j.proba, vp8_coeffs_proba0, sizeof(vp8_coeffs_proba0), hipMemcpyHostToDevice, j.stream);
    int r = hip_rc(e, "hipMemcpyAsync (frames to device)");
    if (r == WG_OK) r = wg_import_rgba(j.rgba, w, h, 4 * w, rgba_b, has_alpha, j.y, j.u, j.v, y_b, uv_b, nk, st);
    if (r == WG_OK) r = wg_analysis_alphas(j.y, j.u, j.v, w, h, y_b, uv_b, nk, j.alphas, nullptr, nullptr, j.uv_sum, st);
    if (r == WG_OK) r = wg_segment_analysis(cfg, j.alphas, j.uv_sum, mbw, mbh, nk, j.seg_ids, j.segs, seg_pitch, j.info, st);
    if (r == WG_OK) r = wg_encode_row_order(j.alphas, mbw, mbh, nk, j.work, st);
    if (r == WG_OK)
      r = wg_encode_mbs(j.y, j.u, j.v, y_b, uv_b, w, h, nk, j.seg_ids, j.segs, seg_pitch, j.proba, cfg->method,
                        cfg->quality, j.out, j.ry, j.ru, j.rv, j.work, st);
    return r;
  });
  // the gather: each device's frames back to their places in the host
  // buffers, enqueued on every device first (the copies of one device overlap
  // the others' kernels and copies), then each stream synchronised and its
  // in-kernel wait status checked (a timed-out launch invalidates the outputs)
  rc = each_lane(jobs, rc, [&](EncLane& j) {
    const struct {
      void* host;  // (an output the caller did not ask for is NULL)
      const void* dev;
      int64_t bytes;  // per frame
    } outs[] = {{mb_out, j.out, rec_b}, {ry, j.ry, y_b}, {ru, j.ru, uv_b}, {rv, j.rv, uv_b}, {seg_ids_out, j.seg_ids, n_mb},
                {info_out, j.info, (int64_t)sizeof(wg_frame_segs)}};
    hipError_t e = hipSuccess;
    for (size_t q = 0; q < j.frames.size(); q++)
      for (const auto& o : outs)
        if (o.host && e == hipSuccess)
          e = hipMemcpyAsync(static_cast<uint8_t*>(o.host) + j.frames[q] * o.bytes,
                             static_cast<const uint8_t*>(o.dev) + (int64_t)q * o.bytes, (size_t)o.bytes,
                             hipMemcpyDeviceToHost, j.stream);
    return hip_rc(e, "gather (device to host)");
  });
  return each_lane(jobs, rc, [&](EncLane& j) {  // (the status call synchronises the stream)
    return wg_encode_status(j.work, mbw, (int)j.frames.size(), j.stream);
  });
}

// ---------------- one large image over several devices: row bands (C5) ----------------
//
// the streaming stages of C5 shard by row bands with a halo --
// VP8L ResidualImage by tile rows (1 pixel row above the band: the
// predictors read the row above), plane SSIM by 16-row tiles (3 rows each
// side).  Device k of n takes the contiguous tile-row band band_of(k) (the
// first tiles % n devices one tile row more, as webp_amd/shard.py band_of),
// computes it through the *_rows entry points from its rows plus the halo,
// and the bands come back to host memory at their places.  The SSIM bands'
// per-tile partial sums are reduced on the first device in the one-device
// order, so the sum is bit-identical to wg_plane_ssim's.
namespace {

struct Band : Lane {
  int t0 = 0, t1 = 0;  // its tile rows: band k of n
  void band_of(int tiles, int n, int k) {
    t0 = k * (tiles / n) + std::min(k, tiles % n);
    t1 = t0 + tiles / n + (k < tiles % n ? 1 : 0);
  }
};

}  // namespace

extern "C" int wg_vp8l_residual_image_devices(const int32_t* devices, int32_t n_devices, const uint32_t* argb,
                                              int32_t width, int32_t height, int32_t bits, int32_t quality,
                                              uint32_t* modes, uint32_t* residuals) {
  WG_REQUIRE(devices && n_devices > 0 && argb && modes && residuals);
  WG_REQUIRE(width > 0 && height > 0 && bits >= 2 && bits <= 9);
  if (int rc = check_devices(devices, n_devices)) return rc;
  const int ts = 1 << bits, tx = (width + ts - 1) >> bits, ty = (height + ts - 1) >> bits;
  const int64_t px = (int64_t)width * height, row_b = (int64_t)width * 4;
  DeviceGuard guard;
  if (guard.save() != hipSuccess) return wg::check_launch("hipGetDevice");
  HostPins pins;
  pins.pin(argb, (size_t)(px * 4));
  pins.pin(modes, (size_t)tx * ty * 4);
  pins.pin(residuals, (size_t)(px * 4));
  // a band's buffers: its rows of the image from h0 (the row above its first,
  // which the predictors read), its residual rows likewise, its tile modes
  struct ResBand : Band {
    int h0, r0, r1;
    uint32_t *in, *res, *modes;
  };
  std::vector<ResBand> bands((size_t)n_devices);
  int rc = WG_OK;
  for (int k = 0; k < n_devices && rc == WG_OK; k++) {
    ResBand& b = bands[(size_t)k];
    b.band_of(ty, n_devices, k);
    if (b.t1 <= b.t0) continue;
    b.r0 = b.t0 << bits, b.r1 = std::min(b.t1 << bits, (int)height), b.h0 = b.r0 - (b.t0 > 0 ? 1 : 0);
    const size_t in_b = (size_t)((b.r1 - b.h0) * row_b);
    hipError_t e = b.open(devices[k], [&] {
      b.in = b.take<uint32_t>(in_b);
      b.res = b.take<uint32_t>(in_b);
      b.modes = b.take<uint32_t>((size_t)tx * (b.t1 - b.t0) * 4);
    });
    if (e == hipSuccess) e = hipMemcpyAsync(b.in, argb + (int64_t)b.h0 * width, in_b, hipMemcpyHostToDevice, b.stream);
    if ((rc = hip_rc(e, "device setup (residual bands)")) != WG_OK) break;
    // the *_rows entry points address rows at their image positions, so they
    // get base pointers moved back by the buffer's first row / tile row (only
    // the band's own rows are ever touched)
    rc = wg_vp8l_residual_image_rows(b.in - (int64_t)b.h0 * width, width, height, px, bits, quality, b.t0, b.t1, 1,
                                     b.modes - (int64_t)b.t0 * tx, b.res - (int64_t)b.h0 * width, b.stream);
  }
  // gather: the band's tile modes and residual rows at their places
  rc = each_lane(bands, rc, [&](ResBand& b) {
    hipError_t e = hipMemcpyAsync(modes + (int64_t)b.t0 * tx, b.modes, (size_t)(b.t1 - b.t0) * tx * 4,
                                  hipMemcpyDeviceToHost, b.stream);
    if (e == hipSuccess)
      e = hipMemcpyAsync(residuals + (int64_t)b.r0 * width, b.res + (int64_t)(b.r0 - b.h0) * width,
                         (size_t)((b.r1 - b.r0) * row_b), hipMemcpyDeviceToHost, b.stream);
    return hip_rc(e, "gather (residual bands)");
  });
  return wait_lanes(bands, rc, "gather (residual bands)");
}

extern "C" int wg_plane_ssim_devices(const int32_t* devices, int32_t n_devices, const uint8_t* a, int32_t a_stride,
                                     const uint8_t* b_plane, int32_t b_stride, int32_t w, int32_t h, double* out) {
  WG_REQUIRE(devices && n_devices > 0 && a && b_plane && out);
  WG_REQUIRE(w > 0 && h > 0 && a_stride >= w && b_stride >= w);
  if (int rc = check_devices(devices, n_devices)) return rc;
  constexpr int TILE = 16, HALO = 3;
  const int tx = wg_plane_ssim_row_partials(w), ty = (h + TILE - 1) / TILE;  // partials per tile row, tile rows
  DeviceGuard guard;
  if (guard.save() != hipSuccess) return wg::check_launch("hipGetDevice");
  std::vector<double> partial((size_t)tx * ty);
  HostPins pins;  // (declared after `partial`: unpinned before it is freed)
  pins.pin(a, (size_t)a_stride * h);
  pins.pin(b_plane, (size_t)b_stride * h);
  pins.pin(partial.data(), partial.size() * sizeof(double));
  // a band's buffers: its rows + halo of both planes, its partial sums (band 0: + all of them and the sum)
  struct SsimBand : Band {
    uint8_t *a, *b;
    double *part, *all, *sum;
  };
  std::vector<SsimBand> bands((size_t)n_devices);
  int rc = WG_OK;
  for (int k = 0; k < n_devices && rc == WG_OK; k++) {
    SsimBand& b = bands[(size_t)k];
    b.band_of(ty, n_devices, k);
    if (b.t1 <= b.t0) continue;
    const int r0 = std::max(TILE * b.t0 - HALO, 0), r1 = std::min(TILE * b.t1 + HALO, (int)h);
    hipError_t e = b.open(devices[k], [&] {
      b.a = b.take<uint8_t>((size_t)(r1 - r0) * a_stride);
      b.b = b.take<uint8_t>((size_t)(r1 - r0) * b_stride);
      b.part = b.take<double>((size_t)tx * (b.t1 - b.t0) * sizeof(double));
      b.all = b.take<double>(k == 0 ? partial.size() * sizeof(double) : 0);
      b.sum = b.take<double>(k == 0 ? sizeof(double) : 0);
    });
    if (e == hipSuccess)
      e = hipMemcpyAsync(b.a, a + (size_t)r0 * a_stride, (size_t)(r1 - r0) * a_stride, hipMemcpyHostToDevice, b.stream);
    if (e == hipSuccess)
      e = hipMemcpyAsync(b.b, b_plane + (size_t)r0 * b_stride, (size_t)(r1 - r0) * b_stride, hipMemcpyHostToDevice,
                         b.stream);
    if ((rc = hip_rc(e, "device setup (ssim bands)")) != WG_OK) break;
    // plane bases moved back by r0 rows: the rows entry point addresses rows at their image positions
    rc = wg_plane_ssim_rows(b.a - (int64_t)r0 * a_stride, a_stride, (int64_t)a_stride * h,
                            b.b - (int64_t)r0 * b_stride, b_stride, (int64_t)b_stride * h, w, h, b.t0, b.t1, 1, b.part,
                            b.stream);
  }
  // gather the per-tile partial sums in tile-row order
  rc = each_lane(bands, rc, [&](SsimBand& b) {
    return hip_rc(hipMemcpyAsync(partial.data() + (size_t)b.t0 * tx, b.part, (size_t)tx * (b.t1 - b.t0) * sizeof(double),
                                 hipMemcpyDeviceToHost, b.stream),
                  "gather (ssim bands)");
  });
  rc = wait_lanes(bands, rc, "gather (ssim bands)");
  if (rc != WG_OK) return rc;
  // the one-device reduction order, on the first device (band 0 is never empty)
  SsimBand& b = bands[0];
  hipError_t e = hipSetDevice(b.dev);
  if (e == hipSuccess) e = hipMemcpyAsync(b.all, partial.data(), partial.size() * sizeof(double), hipMemcpyHostToDevice, b.stream);
  if (e == hipSuccess) rc = wg_plane_ssim_reduce(b.all, (int64_t)partial.size(), 1, b.sum, b.stream);
  if (e == hipSuccess && rc == WG_OK) e = hipMemcpyAsync(out, b.sum, sizeof(double), hipMemcpyDeviceToHost, b.stream);
  if (e == hipSuccess && rc == WG_OK) e = hipStreamSynchronize(b.stream);
  return rc != WG_OK ? rc : hip_rc(e, "ssim reduce");
}
