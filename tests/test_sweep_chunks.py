"""csrc/fic_sweep_chunks.h, the pool-chunk rules of every sweep but the matrix-core least-squares ones, as a program of its own
(tests/cpp/sweep_chunks_test.cpp) against tests/golden/sweep_chunks.txt and the properties the launchers rely on."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sweep_chunk_rules_under_the_sanitizers(tmp_path):
    """Built with the host compiler's address and undefined-behaviour sanitizers where it has their runtimes."""
    src = os.path.join(ROOT, "tests", "cpp", "sweep_chunks_test.cpp")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    ok = subprocess.run(["g++"] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode == 0
    if not ok or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        san = []
    print("sweep_chunks_test built " + ("with " + san[0] if san else "WITHOUT sanitizers (the host compiler has no runtimes for them)"))
    exe = str(tmp_path / "sweep_chunks_test")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + san + [src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "sweep_chunks.txt")], capture_output=True, text=True)
    assert r.returncode == 0 and "\n0 failures" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr
    assert "1620 recorded rows compared" in r.stdout
