"""csrc/fic_qt_decode_plan.h, the decode side of a batched quadtree context, as a program of its own
(tests/cpp/qt_decode_plan_test.cpp): the layout of the decode store, and the closed form of a leaf's place among the decoder's
squares against a plain walk of the tree in the stream parser's order."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_decode_plan_under_the_sanitizers(tmp_path):
    """Built with the host compiler's address and undefined-behaviour sanitizers where it has their runtimes; the program
    runs as its own executable."""
    src = os.path.join(ROOT, "tests", "cpp", "qt_decode_plan_test.cpp")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    ok = subprocess.run(["g++"] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode == 0
    if not ok or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        san = []
    print("qt_decode_plan_test built " + ("with " + san[0] if san else "WITHOUT sanitizers (the host compiler has no runtimes for them)"))
    exe = str(tmp_path / "qt_decode_plan_test")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + san + [src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "\n0 failures" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr
    # 4 shapes x 3 plane counts x 2 pixel sizes x 3 zooms; 3 ladders x 3 zooms x (17 + 2 + 2) / 3 trees + 4 shapes x 3 zooms x 20
    assert "72 plans checked" in r.stdout and "303 trees walked" in r.stdout
