#!/usr/bin/env python3
"""Wall-clock timings of the streams with an isometry column through their C entry points (host buffers in and out, warm
caches) on LenaColored enlarged to 512x512 and 2048x2048: the colour quadtree encode 16 -> 4 with n_iso = 1 and 8 (full search,
threshold 400) against the fixed-B n_iso = 8 one-shot encodes it is built from and against the existing colour quadtree, the
decode of its tag-6 stream, the decode of the tag-5 stream of the B = 8 codebook, and the leaf counts.  Medians of `reps`
calls.  Never bench.py's `value`.  Usage: iso_stream_timing.py [out.json]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fic_amd  # noqa: E402
from fic_amd import capi, synth  # noqa: E402

T = 400.0


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def psnr(img, rgb):
    u = img.view(np.uint32)
    got = np.stack([(u >> 16) & 0xFF, (u >> 8) & 0xFF, u & 0xFF], axis=-1).astype(np.float64)
    d = got.reshape(rgb.shape) - rgb
    return float(10 * np.log10(255.0 ** 2 / np.mean(d * d)))


lena = np.load(os.path.join(ROOT, "tests", "golden", "lena_colored_256.npy"))
out = {}
for W, reps in ((512, 10), (2048, 5)):
    rgb = np.stack([synth.enlarge(np.ascontiguousarray(lena[..., c]), W, W) for c in range(3)], axis=-1)
    c = rgb.astype(np.uint32)
    argb = (0xFF000000 | (c[..., 0] << 16) | (c[..., 1] << 8) | c[..., 2]).view(np.int32).reshape(-1)
    Dw = {B: capi.geometry(W, W, B)[2] for B in (16, 8, 4)}
    res = {"threshold": T, "reps": reps}
    for n_iso in (1, 8):
        for _ in range(2):                                  # code objects, working sets, first-touch pages
            leaves = fic_amd.encode_rgb_quadtree_iso(argb, W, W, 16, 4, 0, n_iso, T)
        enc = median_ms(lambda: fic_amd.encode_rgb_quadtree_iso(argb, W, W, 16, 4, 0, n_iso, T), reps)
        fixed = {B: median_ms(lambda: capi.encode_rgb(argb, W, W, B, Dw[B], n_iso=n_iso), reps) for B in (16, 8, 4)}
        run = fic_amd.write_run_rgb_quadtree_iso(leaves, W, W, 16, 4, 0)
        img, avg, it = fic_amd.decode_rgb_quadtree_iso_run(run)
        dec = median_ms(lambda: fic_amd.decode_rgb_quadtree_iso_run(run), reps)
        res[f"tag6_n_iso{n_iso}"] = {
            "encode_16_4_ms": enc, "fixed_oneshot_ms": {str(B): v for B, v in fixed.items()}, "fixed_sum_ms": sum(fixed.values()),
            "encode_over_fixed_sum": enc / sum(fixed.values()), "decode_ms": dec, "iterations": it, "leaves": int(len(leaves)),
            "leaves_per_B": {str(B): int((leaves[:, 2] == B).sum()) for B in (16, 8, 4)}, "stream_bytes": len(run),
            "psnr_db": psnr(img, rgb)}
    # the existing colour quadtree (tag 3, no isometries) on the same image
    for _ in range(2):
        old = fic_amd.encode_rgb_quadtree(argb, W, W, 16, 4, 0, T)
    run3 = fic_amd.write_run_rgb_quadtree(old, W, W, 16, 4, 0)
    img3, _, it3 = fic_amd.decode_rgb_quadtree_run(run3)
    res["tag3"] = {"encode_16_4_ms": median_ms(lambda: fic_amd.encode_rgb_quadtree(argb, W, W, 16, 4, 0, T), reps),
                   "decode_ms": median_ms(lambda: fic_amd.decode_rgb_quadtree_run(run3), reps), "iterations": it3,
                   "leaves": int(len(old)), "stream_bytes": len(run3), "psnr_db": psnr(img3, rgb)}
    # the fixed B = 8, n_iso = 8 codebook as a tag-5 stream, and the tag-1 stream of the n_iso = 1 codebook beside it
    r8 = capi.encode_rgb(argb, W, W, 8, Dw[8], n_iso=8)
    run5 = fic_amd.write_run_rgb_iso(r8["qrows"], r8["iso"], W, W, 8, Dw[8])
    img5, _, it5, _, _ = fic_amd.decode_rgb_iso_run(run5)
    run1 = fic_amd.write_run_rgb(capi.encode_rgb(argb, W, W, 8, Dw[8])["qrows"], W, W, 8, Dw[8])
    img1, _, it1, _, _ = fic_amd.decode_rgb_run(run1)
    res["tag5_B8"] = {"decode_ms": median_ms(lambda: fic_amd.decode_rgb_iso_run(run5), reps), "iterations": it5,
                      "stream_bytes": len(run5), "psnr_db": psnr(img5, rgb),
                      "decode_zoom2_ms": median_ms(lambda: fic_amd.decode_rgb_iso_run(run5, zoom=2), reps)}
    res["tag1_B8"] = {"decode_ms": median_ms(lambda: fic_amd.decode_rgb_run(run1), reps), "iterations": it1,
                      "stream_bytes": len(run1), "psnr_db": psnr(img1, rgb)}
    out[f"{W}x{W}"] = res
    print(W, json.dumps(res), flush=True)
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
