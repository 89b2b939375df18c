#!/usr/bin/env python3
"""Wall-clock timings of the quadtree codec through its C entry points (host buffers in and out, warm caches): encode 16 -> 4
(full search, 1 isometry, threshold 400) against the three fixed-B one-shot encodes it is built from, and the decode of its
stream, on LenaGrey enlarged to 512x512 and 2048x2048.  Medians of `reps` calls.  Never bench.py's `value`.
Usage: quadtree_timing.py [out.json]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fic_amd  # noqa: E402
from fic_amd import capi, synth  # noqa: E402


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


lena = np.load(os.path.join(ROOT, "tests", "golden", "lena_grey_256.npy"))
out = {}
for W, reps in ((512, 10), (2048, 5)):
    g = synth.enlarge(lena, W, W)
    t = 400.0
    for _ in range(2):                                      # code objects, working sets, first-touch pages
        leaves = fic_amd.encode_gray_quadtree(g, 16, 4, 0, 1, t)
    enc = median_ms(lambda: fic_amd.encode_gray_quadtree(g, 16, 4, 0, 1, t), reps)
    fixed = {B: median_ms(lambda: capi.encode_gray_oneshot(g, B, None, 1), reps) for B in (16, 8, 4)}
    run = fic_amd.write_run_quadtree(leaves, W, W, 16, 4, 0, 1)
    img, avg, it = fic_amd.decode_quadtree_run(run)
    dec = median_ms(lambda: fic_amd.decode_quadtree_run(run), reps)
    d = img.astype(np.float64) - g
    out[f"{W}x{W}"] = {
        "encode_16_4_ms": enc, "fixed_oneshot_ms": {str(B): v for B, v in fixed.items()},
        "fixed_sum_ms": sum(fixed.values()), "decode_ms": dec, "iterations": it, "leaves": int(len(leaves)),
        "leaves_per_B": {str(B): int((leaves[:, 2] == B).sum()) for B in (16, 8, 4)},
        "psnr_db": float(10 * np.log10(255.0 ** 2 / np.mean(d * d))), "reps": reps,
    }
    print(W, json.dumps(out[f"{W}x{W}"]), flush=True)
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
