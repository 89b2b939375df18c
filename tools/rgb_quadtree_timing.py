#!/usr/bin/env python3
"""Wall-clock timings of the colour (joint-RGB) quadtree codec through its C entry points (host buffers in and out, warm
caches): encode 16 -> 4 (full search, threshold 1200) against the three fixed-B RGB one-shot encodes it is built from, and
the decode of its stream, on LenaColored enlarged to 512x512 and 2048x2048.  Medians of `reps` calls.  Never bench.py's
`value`.  Usage: rgb_quadtree_timing.py [out.json]"""
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


lena = np.load(os.path.join(ROOT, "tests", "golden", "lena_colored_256.npy"))
out = {}
for W, reps in ((512, 10), (2048, 5)):
    rgb = np.stack([synth.enlarge(np.ascontiguousarray(lena[..., c]), W, W) for c in range(3)], axis=-1)
    c = rgb.astype(np.uint32)
    argb = (0xFF000000 | (c[..., 0] << 16) | (c[..., 1] << 8) | c[..., 2]).view(np.int32).reshape(-1)
    t = 1200.0
    for _ in range(2):                                      # code objects, working sets, first-touch pages
        leaves = fic_amd.encode_rgb_quadtree(argb, W, W, 16, 4, 0, t)
    enc = median_ms(lambda: fic_amd.encode_rgb_quadtree(argb, W, W, 16, 4, 0, t), reps)
    Dw = {B: capi.geometry(W, W, B)[2] for B in (16, 8, 4)}
    fixed = {B: median_ms(lambda: capi.encode_rgb(argb, W, W, B, Dw[B]), reps) for B in (16, 8, 4)}
    run = fic_amd.write_run_rgb_quadtree(leaves, W, W, 16, 4, 0)
    img, avg, it = fic_amd.decode_rgb_quadtree_run(run)
    dec = median_ms(lambda: fic_amd.decode_rgb_quadtree_run(run), reps)
    u = img.view(np.uint32)
    got = np.stack([(u >> 16) & 0xFF, (u >> 8) & 0xFF, u & 0xFF], axis=-1).astype(np.float64)
    d = got - rgb
    out[f"{W}x{W}"] = {
        "encode_16_4_ms": enc, "fixed_oneshot_ms": {str(B): v for B, v in fixed.items()},
        "fixed_sum_ms": sum(fixed.values()), "decode_ms": dec, "iterations": it, "threshold": t, "leaves": int(len(leaves)),
        "leaves_per_B": {str(B): int((leaves[:, 2] == B).sum()) for B in (16, 8, 4)},
        "psnr_db": float(10 * np.log10(255.0 ** 2 / np.mean(d * d))), "reps": reps,
    }
    print(W, json.dumps(out[f"{W}x{W}"]), flush=True)
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
