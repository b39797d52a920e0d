"""CPU: the per-device registry (webp_amd/csrc/wg_device.h) on its own.

tests/per_device_test.cpp includes only that header and has its own main; it
is built with g++ twice -- under ThreadSanitizer, and under AddressSanitizer +
UBSan -- and each binary is run directly (nothing is preloaded, nothing is
loaded into Python).  It checks that 16 threads calling get() for 4 devices at
once run each device's init exactly once and all see the same object, that a
failed init leaves the slot empty so the next get() runs it again, and that
devices -1 and kMaxDevices are refused without running init.

A sanitizer whose runtime cannot be linked here (or cannot start even under
an empty main) skips that build, with the tool's message as the reason."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "per_device_test.cpp")
BASE = ["g++", "-std=c++17", "-pthread", "-O1", "-g", "-Wall", "-Wextra", "-Werror"]


def usable(tmp_path, flag):
    """Whether an empty program links with `flag` and starts (the sanitizer's
    runtime is installed and can set itself up in this process environment)."""
    src, exe = tmp_path / "empty.cpp", str(tmp_path / "empty")
    src.write_text("int main() { return 0; }\n")
    p = subprocess.run(["g++", flag, str(src), "-o", exe], capture_output=True, text=True)
    if p.returncode == 0:
        p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    return p.returncode == 0, p.stderr.strip()[-300:]


@pytest.mark.parametrize("sanitizer", ["thread", "address,undefined"])
def test_per_device_registry_under_sanitizer(tmp_path, sanitizer):
    flag = "-fsanitize=" + sanitizer
    ok, why = usable(tmp_path, flag)
    if not ok:
        pytest.skip(f"g++ cannot link {flag}, or its runtime cannot start, here: {why}")
    exe = str(tmp_path / "per_device_test")
    p = subprocess.run(BASE + [flag, "-fno-sanitize-recover=all", SRC, "-o", exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=100)
    assert p.returncode == 0 and "per_device_test: ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-3000:])
