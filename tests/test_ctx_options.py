"""csrc/fic_ctx_options.h, the option names the three handles share with their ranges and refusals, as a program
of its own (tests/cpp/ctx_options_test.cpp): for every name the two boundaries inside, one step outside on each side, the gap of
lsq_tau_widen, the handles that do not know a name, and an unknown name."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_option_rules_under_the_sanitizers(tmp_path):
    """Built with the host compiler's address and undefined-behaviour sanitizers where it has their runtimes; the program
    runs as its own executable."""
    src = os.path.join(ROOT, "tests", "cpp", "ctx_options_test.cpp")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    ok = subprocess.run(["g++"] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode == 0
    if not ok or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        san = []
    print("ctx_options_test built " + ("with " + san[0] if san else "WITHOUT sanitizers (the host compiler has no runtimes for them)"))
    exe = str(tmp_path / "ctx_options_test")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + san + [src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "\n0 failures" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr
    assert "checks\n" in r.stdout and not r.stdout.startswith("0 checks")
