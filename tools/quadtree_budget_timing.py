#!/usr/bin/env python3
"""Wall-clock timings of the quadtree encode to a leaf budget through its C entry point (host buffers in and out, warm caches)
against the fixed-threshold encode at the threshold the budget chose: LenaGrey enlarged to 512x512 and 2048x2048, 16 -> 4, full
search, 1 isometry, the budget = the leaf count of threshold 400 (the geometries of profiles/quadtree_timing.json).  Medians of
`reps` calls.  A bisection on the threshold from outside needs at least two fixed-threshold encodes; the budget encode is one
encode plus the select.  Never bench.py's `value`.

Usage: quadtree_budget_timing.py [out.txt] [--fixed-root DIR] [--once W]
  --fixed-root DIR   also time the fixed-threshold encode of another checkout of this project (built in place: the commit before
                     the budget entries), in a fresh process that imports DIR's package
  --once W           no timing: a few budget encodes of the W x W image (the workload for a kernel trace)"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIXED_CHILD = """
import json, sys, time
import numpy as np
sys.path.insert(0, sys.argv[1])
import fic_amd
from fic_amd import synth
lena = np.load(sys.argv[2])
out = {}
for W, reps, t in json.loads(sys.argv[3]):
    g = synth.enlarge(lena, W, W)
    for _ in range(2):
        leaves = fic_amd.encode_gray_quadtree(g, 16, 4, 0, 1, t)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fic_amd.encode_gray_quadtree(g, 16, 4, 0, 1, t)
        ts.append((time.perf_counter() - t0) * 1e3)
    out[str(W)] = {"ms": float(np.median(ts)), "leaves": int(len(leaves))}
print(json.dumps(out))
"""


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main(argv):
    out_path = fixed_root = once = None
    it = iter(argv)
    for a in it:
        if a == "--fixed-root":
            fixed_root = os.path.abspath(next(it))
        elif a == "--once":
            once = int(next(it))
        else:
            out_path = a
    sys.path.insert(0, ROOT)
    import fic_amd
    from fic_amd import synth
    golden = os.path.join(ROOT, "tests", "golden", "lena_grey_256.npy")
    lena = np.load(golden)
    if once:
        g = synth.enlarge(lena, once, once)
        M = len(fic_amd.encode_gray_quadtree(g, 16, 4, 0, 1, 400.0))
        for _ in range(5):
            leaves, t, stats = fic_amd.encode_gray_quadtree_budget(g, 16, 4, 0, 1, max_leaves=M)
        print(once, M, len(leaves), float(t), stats.tolist())
        return
    rows, jobs = [], []
    for W, reps in ((512, 20), (2048, 10)):
        g = synth.enlarge(lena, W, W)
        M = len(fic_amd.encode_gray_quadtree(g, 16, 4, 0, 1, 400.0))
        for _ in range(2):                                  # code objects, working sets, first-touch pages
            leaves, t, stats = fic_amd.encode_gray_quadtree_budget(g, 16, 4, 0, 1, max_leaves=M)
            fixed = fic_amd.encode_gray_quadtree(g, 16, 4, 0, 1, t)
        assert (leaves == fixed).all() and len(leaves) <= M
        r = {"image": f"{W}x{W}", "max_leaves": M, "threshold": float(t), "leaves": int(len(leaves)), "collage_sse": int(stats[0]),
             "leaves_per_B": {str(16 >> l): int(stats[1 + l]) for l in range(3)}, "reps": reps}
        # interleaved, so that a drift of the clock reaches both alike
        b, f = [], []
        for _ in range(reps):
            b.append(median_ms(lambda: fic_amd.encode_gray_quadtree_budget(g, 16, 4, 0, 1, max_leaves=M), 1))
            f.append(median_ms(lambda: fic_amd.encode_gray_quadtree(g, 16, 4, 0, 1, t), 1))
        r["budget_ms"], r["fixed_ms"] = float(np.median(b)), float(np.median(f))
        rows.append(r)
        jobs.append((W, reps, float(t)))
    if fixed_root:
        res = subprocess.run([sys.executable, "-c", FIXED_CHILD, fixed_root, golden, json.dumps(jobs)], capture_output=True, text=True,
                             timeout=600, env={k: v for k, v in os.environ.items() if k != "FIC_HIP_SO"})
        if res.returncode:
            raise RuntimeError(f"fixed-threshold timing in {fixed_root} failed:\n{res.stderr}")
        other = json.loads(res.stdout.strip().splitlines()[-1])
        for r, (W, _, _) in zip(rows, jobs):
            assert other[str(W)]["leaves"] == r["leaves"]
            r["fixed_other_checkout_ms"] = other[str(W)]["ms"]
    lines = []
    for r in rows:
        ref = r.get("fixed_other_checkout_ms", r["fixed_ms"])
        r["budget_over_fixed"] = r["budget_ms"] / ref
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
