// Stand-alone check of wg::PerDevice (webp_amd/csrc/wg_device.h), built by
// tests/test_per_device.py with g++ under ThreadSanitizer and under
// AddressSanitizer + UBSan and run directly.  Exit status 0 iff every check
// holds; each failed check is printed.
#include <atomic>
#include <cstdio>
#include <thread>
#include <vector>

#include "../webp_amd/csrc/wg_device.h"

namespace {
int failures = 0;
void expect(bool ok, const char* what) {
  if (!ok) {
    std::printf("FAILED: %s\n", what);
    failures++;
  }
}
struct Record {
  int dev;
  int payload[8];
};
}  // namespace

int main() {
  constexpr int kThreads = 16, kDevices = 4, kRounds = 50;
  {  // concurrent first calls: one init per device, one object per device
    wg::PerDevice<Record> reg;
    std::atomic<int> inits[kDevices];
    for (auto& n : inits) n = 0;
    std::atomic<int> ready{0};
    Record* seen[kThreads][kDevices] = {};
    bool filled[kThreads] = {};
    std::vector<std::thread> ths;
    for (int t = 0; t < kThreads; t++)
      ths.emplace_back([&, t] {
        ready++;
        while (ready.load() < kThreads) std::this_thread::yield();  // first calls together
        bool ok = true;
        for (int r = 0; r < kRounds; r++)
          for (int k = 0; k < kDevices; k++) {
            const int dev = (k + t) % kDevices;
            Record* p = reg.get(dev, [&](Record& rec) {
              inits[dev]++;
              rec.dev = dev;
              for (int i = 0; i < 8; i++) rec.payload[i] = 100 * dev + i;  // plain writes: the lock publishes them
              return true;
            });
            ok = ok && p && p->dev == dev && p->payload[7] == 100 * dev + 7 && (!seen[t][dev] || seen[t][dev] == p);
            seen[t][dev] = p;
          }
        filled[t] = ok;
      });
    for (auto& th : ths) th.join();
    for (int k = 0; k < kDevices; k++) expect(inits[k] == 1, "init ran exactly once per device");
    for (int t = 0; t < kThreads; t++) {
      expect(filled[t], "every get returned its device's initialised record");
      for (int k = 0; k < kDevices; k++) expect(seen[t][k] == seen[0][k], "all threads see the same object");
    }
    expect(seen[0][0] != seen[0][1], "devices have records of their own");
  }
  {  // a failed init leaves the slot empty; the next get runs it again
    wg::PerDevice<int> reg;
    int runs = 0;
    auto init = [&](int& v) {
      v = 7;
      return ++runs >= 2;
    };
    expect(reg.get(3, init) == nullptr && runs == 1, "a failed init gives nullptr");
    int* p = reg.get(3, init);
    expect(p && *p == 7 && runs == 2, "the next get runs init again");
    expect(reg.get(3, init) == p && runs == 2, "and then never again");
  }
  {  // out of range: refused, init not run
    wg::PerDevice<int> reg;
    int runs = 0;
    auto init = [&](int&) { return ++runs > 0; };
    expect(reg.get(-1, init) == nullptr && reg.get(wg::kMaxDevices, init) == nullptr && runs == 0,
           "devices -1 and kMaxDevices are refused without running init");
    reg.update(-1, [&](int&) { runs++; });
    reg.update(wg::kMaxDevices, [&](int&) { runs++; });
    expect(runs == 0, "update refuses them too");
    expect(reg.get(wg::kMaxDevices - 1, init) != nullptr && runs == 1, "the last device is served");
    reg.update(wg::kMaxDevices - 1, [](int& v) { v = 42; });
    expect(*reg.get(wg::kMaxDevices - 1, init) == 42 && runs == 1, "update changes the record get returns");
  }
  std::printf("%s\n", failures ? "per_device_test: FAILED" : "per_device_test: ok");
  return failures ? 1 : 0;
}
