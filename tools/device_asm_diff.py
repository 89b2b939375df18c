#!/usr/bin/env python3
"""Does a change to a .hip file change the device code?  Per-kernel comparison of two source trees.

    tools/device_asm_diff.py NEW_TREE OLD_TREE fic_q.hip [--cflags="-DFIC_Q_PHASES"] [--no-xcheck] [--keep DIR]

Compiles csrc/<file> of both trees to gfx950 assembly with each tree's own build.py FLAGS (read from that file, not
copied here) plus --cuda-device-only -S, drops the __hip_cuid_ lines (the symbol hashes the source text), and reports for
every kernel whether its text -- everything up to and including its .amdhsa_kernel descriptor -- and its entry in the
metadata block are the same on both sides.  For a kernel that differs it prints both sides' VGPR, SGPR, scratch and LDS
figures.  CPU only: hipcc cross-compiles.  Exit status 1 when any kernel differs.
"""
import argparse
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

PKG = "fractal-image-compression_amd"


def load_build(tree):
    spec = importlib.util.spec_from_file_location("fic_build_" + str(abs(hash(tree))), os.path.join(tree, PKG, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def compile_asm(tree, src, extra, xcheck, out):
    b = load_build(tree)
    flags = [f for f in b.FLAGS if f != "-shared"]           # a link flag: nothing is linked here
    cmd = ([b._hipcc()] + flags + (["-DFIC_BUILD_XCHECK"] if xcheck else []) + extra +
           ["--cuda-device-only", "-S", src, "-o", out])
    subprocess.check_call(cmd, cwd=b.CSRC)
    with open(out) as f:
        return [ln.rstrip("\n") for ln in f if "__hip_cuid_" not in ln]


def split_kernels(lines):
    """{kernel: its text}, the kernels' order, {kernel: its metadata entry}.  A kernel's text runs from its "Begin function"
    line to the next kernel's: the code, the .amdhsa_kernel descriptor and the register summary behind it.  What stands
    before the first kernel and between the last one's summary and the metadata is compared as '<tail>'."""
    text, order, name, described = {"<tail>": []}, [], "<tail>", False
    meta_at = next((i for i, ln in enumerate(lines) if ln.strip() == ".amdgpu_metadata"), len(lines))
    for ln in lines[:meta_at]:
        m = re.search(r";\s*-- Begin function\s+(\S+)", ln)
        if m:
            name, described = m.group(1), False
            text[name] = []
            order.append(name)
        elif ln.strip() == ".end_amdhsa_kernel":
            described = True
        elif described and re.match(r"\s*\.section\s", ln) and ".AMDGPU.csdata" not in ln and ".text." + name + "," not in ln:
            name, described = "<tail>", False                # the next kernel's section line, or the sections behind the last kernel
        text[name].append(ln)
    meta, entry = {}, None
    for ln in lines[meta_at:]:
        if ln.startswith("  - "):                            # an element of amdhsa.kernels
            entry = [ln]
        elif entry is not None and ln.startswith("    "):
            entry.append(ln)
            m = re.match(r"\s+\.name:\s+(\S+)", ln)
            if m:
                meta[m.group(1)] = entry
        else:
            entry = None
    return text, order, meta


def figures(entry):
    get = lambda key: next((int(m.group(1)) for ln in entry or [] for m in [re.match(r"\s+(?:- )?\." + key + r":\s+(\d+)", ln)] if m), -1)
    return "vgpr %d sgpr %d scratch %d lds %d" % (get("vgpr_count"), get("sgpr_count"), get("private_segment_fixed_size"),
                                                  get("group_segment_fixed_size"))


def demangle(names):
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if filt is None:
        return {n: n for n in names}
    out = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, out))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("new_tree")
    ap.add_argument("old_tree")
    ap.add_argument("hip_file", help="a file of csrc/, e.g. fic_q.hip")
    ap.add_argument("--cflags", default="", help="extra compiler flags for both sides, e.g. \"-DFIC_Q_SEED=0\" or \"-O2\"")
    ap.add_argument("--no-xcheck", action="store_true", help="compile without -DFIC_BUILD_XCHECK (the FIC_BUILD_XCHECK=0 build)")
    ap.add_argument("--keep", help="keep the two assembly files in this directory")
    a = ap.parse_args()
    keep = a.keep or tempfile.mkdtemp(prefix="device_asm_diff_")
    os.makedirs(keep, exist_ok=True)
    stem = os.path.splitext(a.hip_file)[0]
    try:
        with ThreadPoolExecutor(2) as ex:
            jobs = [ex.submit(compile_asm, os.path.abspath(t), a.hip_file, a.cflags.split(), not a.no_xcheck,
                              os.path.join(keep, "%s_%s.s" % (stem, side)))
                    for t, side in ((a.new_tree, "new"), (a.old_tree, "old"))]
            new, old = (split_kernels(j.result()) for j in jobs)
    finally:
        if not a.keep:
            shutil.rmtree(keep, ignore_errors=True)
    names = old[1] + [n for n in new[1] if n not in old[0]]
    pretty = demangle(names)
    print("# %s, flags: build.py FLAGS%s%s" % (a.hip_file, "" if a.no_xcheck else " -DFIC_BUILD_XCHECK", " " + a.cflags if a.cflags else ""))
    differ = 0
    for n in names:
        if n not in new[0] or n not in old[0]:
            verdict = "only in the %s tree" % ("old" if n in old[0] else "new")
        elif new[0][n] == old[0][n] and new[2].get(n) == old[2].get(n):
            verdict = "identical"
        else:
            verdict = "DIFFERS  new: %s | old: %s" % (figures(new[2].get(n)), figures(old[2].get(n)))
        differ += verdict != "identical"
        print("%-9s %s" % ("identical", pretty[n]) if verdict == "identical" else "%s\n          %s" % (pretty[n], verdict))
    tail_same = new[0]["<tail>"] == old[0]["<tail>"]
    print("# %d kernels, %d identical, %d not; text outside the kernels %s" %
          (len(names), len(names) - differ, differ, "identical" if tail_same else "differs"))
    return 0 if differ == 0 and tail_same else 1


if __name__ == "__main__":
    sys.exit(main())
