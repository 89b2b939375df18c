"""CPU-side check of fic_quadtree_leaves_for_bytes (csrc/fic_stream.cpp), the byte limit of the quadtree encode to a budget
(DESIGN.md section 4.18): the stand-alone program tests/cpp/stream_budget_test.cpp runs it for every tag and n_iso over byte
limits up to the ends of int64 under AddressSanitizer and UndefinedBehaviorSanitizer, and against the tag's own writer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_leaves_for_bytes_under_sanitizers(tmp_path):
    """Nothing of the program is loaded into this process, and it never runs on a GPU."""
    src = [os.path.join(ROOT, "tests", "cpp", "stream_budget_test.cpp"), os.path.join(ROOT, "fractal-image-compression_amd", "csrc", "fic_stream.cpp")]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    built = subprocess.run(["g++"] + SANITIZE + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode == 0
    if not built or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the host compiler has no sanitizer runtimes, or a program built with them does not start here")
    exe = str(tmp_path / "stream_budget_test")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + SANITIZE + src + ["-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 failures" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr
