"""CPU-side checks of who owns device memory under the C ABI (csrc/fic_devmem.h): the owner's bookkeeping builds with the plain
host compiler, no ROCm include path, and the stand-alone program tests/cpp/devmem_test.cpp runs it on a malloc-backed binding
under AddressSanitizer (with its leak checker) and UndefinedBehaviorSanitizer; and the counters of the library itself stay at
zero when a context is refused."""
import os
import subprocess

import pytest

from fic_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_owner_bookkeeping_under_sanitizers(tmp_path):
    """ensure is idempotent, release nulls and uncounts, bytes_of answers for live pointers only, a failing k-th allocation of ten
    leaves the others usable and is retried, destruction and an early return free everything, the counters end at zero -- and
    an owner that is never destroyed ends the run with the leak checker's error.  Nothing of the program is loaded into this
    process, and it never runs on a GPU."""
    src = [os.path.join(ROOT, "tests", "cpp", "devmem_test.cpp"), os.path.join(ROOT, "fractal-image-compression_amd", "csrc", "fic_stream.cpp")]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    built = subprocess.run(["g++"] + SANITIZE + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode == 0
    if not built or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the host compiler has no sanitizer runtimes, or a program built with them does not start here")
    exe = str(tmp_path / "devmem_test")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + SANITIZE + src + ["-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 failures" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr
    r = subprocess.run([exe, "forget"], capture_output=True, text=True)
    assert "forgot 1000 bytes" in r.stdout and r.returncode != 0 and "LeakSanitizer" in r.stderr, r.stdout + r.stderr


def test_live_memory_is_zero_after_a_refused_create():
    """Without a device fic_ctx_create refuses before it allocates: nothing is live, of either kind."""
    L = capi.lib()
    if L.fic_device_count() > 0:
        pytest.skip("a HIP device is present")
    assert not L.fic_ctx_create(0, 64, 64, 4, 29, 1, 1)
    assert L.fic_last_error_code() == -4 and "no HIP device" in capi.last_error()
    assert not L.fic_rgb_ctx_create_iso(0, 64, 64, 4, 29, 1, 1)
    assert capi.live_memory() == {"device_bytes": 0, "device_allocations": 0, "pinned_bytes": 0, "pinned_allocations": 0}
    assert L.fic_debug_live_memory(None) == -3
