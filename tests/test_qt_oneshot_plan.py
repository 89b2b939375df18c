"""The one-shot quadtree entries run on csrc/fic_qt_batch_plan.h's plan of one plane: it must take the largest
images they take, for every ladder and leaf width (tests/cpp/qt_oneshot_plan_test.cpp, a program of its own)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_one_plane_plan_takes_the_largest_images(tmp_path):
    """Built with the host compiler's address and undefined-behaviour sanitizers where it has their runtimes; the program
    runs as its own executable."""
    src = os.path.join(ROOT, "tests", "cpp", "qt_oneshot_plan_test.cpp")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    ok = subprocess.run(["g++"] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode == 0
    if not ok or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        san = []
    print("qt_oneshot_plan_test built " + ("with " + san[0] if san else "WITHOUT sanitizers (the host compiler has no runtimes for them)"))
    exe = str(tmp_path / "qt_oneshot_plan_test")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + san + [src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "\n0 failures" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr
    assert "27 one-plane plans at the largest images checked" in r.stdout
