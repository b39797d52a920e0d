// runtime.hip -- library-wide C-ABI entry points (error reporting, version,
// device check) and the per-device plumbing of wg_common.h.  There is
// deliberately no CPU fallback anywhere in libwebpgpu.so: a missing /
// non-gfx950 device is an error.
#include <string.h>

#include "wg_common.h"

namespace wg {
static thread_local std::string g_last_error;
void set_error(const std::string& msg) { g_last_error = msg; }

int stream_device(hipStream_t s, int* dev) {
  hipDevice_t d = 0;
  // the null stream is the current device's (hipStreamGetDevice says so too)
  if ((s ? hipStreamGetDevice(s, &d) : hipGetDevice(&d)) != hipSuccess || d < 0 || d >= kMaxDevices) {
    set_error("stream_device: cannot tell the stream's device");
    return WG_EHIP;
  }
  *dev = d;
  return WG_OK;
}

int call_device(hipStream_t s, const char* entry, int* dev) {
  int cur = 0;
  if (const int rc = stream_device(s, dev)) return rc;
  if (hipGetDevice(&cur) != hipSuccess) return check_launch("hipGetDevice");
  return cur == *dev ? WG_OK : invalid((std::string(entry) + ": the stream's device is not the current device").c_str());
}

int device_cus(int dev) {
  static PerDevice<int> cus;
  const int* n = cus.get(dev, [&](int& out) {
    return hipDeviceGetAttribute(&out, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && out > 0;
  });
  if (!n) (void)check_launch("device query (compute units)");
  return n ? *n : 0;
}

namespace {
// per device: the block of diag_words and, per kernel family, the count of
// timed-out waits the status entry points have already reported (diag[0] is
// cumulative on the device)
struct DiagRecord {
  int* block;
  int reported[4];
};
PerDevice<DiagRecord> g_diag;
}  // namespace

// one 64-int block per device -- the device the stream `s` belongs to --
// zeroed once on that stream (a queue already in use: no new hardware queue
// is created for it)
int* diag_words(hipStream_t s, int family) {
  int dev = 0;
  if (stream_device(s, &dev) != WG_OK) return nullptr;
  const DiagRecord* r = g_diag.get(dev, [&](DiagRecord& d) {
    return hipMalloc(&d.block, 64 * sizeof(int)) == hipSuccess &&
           hipMemsetAsync(d.block, 0, 64 * sizeof(int), s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
  });
  if (!r) set_error("diag_words: allocation failed");
  return r ? r->block + family : nullptr;
}

int take_new_timeouts(hipStream_t s, int family, int total) {
  int dev = 0, fresh = total;
  if (stream_device(s, &dev) != WG_OK) return total;
  g_diag.update(dev, [&](DiagRecord& d) {
    int& seen = d.reported[(family / 16) & 3];
    fresh = total - seen;
    seen = total;
  });
  return fresh > 0 ? fresh : 0;
}

namespace {
__global__ void k_inject_timeout(int* diag) { note_timeout(diag, -1, -1, -1, -1, -1, -1); }
}  // namespace
}  // namespace wg

extern "C" int wg_debug_inject_timeout(int32_t family, void* stream) {
  WG_REQUIRE(family == wg::DIAG_ENCODE || family == wg::DIAG_DECODE || family == wg::DIAG_VP8L_INVERSE ||
             family == wg::DIAG_ALPHA);
  hipStream_t s = wg::as_stream(stream);
  int* diag = wg::diag_words(s, family);
  if (!diag) return WG_EHIP;
  hipLaunchKernelGGL(wg::k_inject_timeout, dim3(1), dim3(1), 0, s, diag);
  return wg::check_launch("k_inject_timeout");
}

extern "C" const char* wg_last_error(void) { return wg::g_last_error.c_str(); }

extern "C" int wg_version(void) { return WG_ABI_VERSION; }

extern "C" int wg_device_check(void) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) {
    wg::set_error("hipGetDevice failed: no HIP device");
    return WG_ENODEV;
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) {
    wg::set_error("hipGetDeviceProperties failed");
    return WG_ENODEV;
  }
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    wg::set_error(std::string("unsupported device arch: ") + prop.gcnArchName + " (built for gfx950)");
    return WG_ENODEV;
  }
  return WG_OK;
}
