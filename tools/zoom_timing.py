"""Timing of a decode at zoom 4 against a native decode of the same size: a 1024x1024, B = 16 stream
decoded at zoom 4 (4096x4096 out, block side 64) and the stream of a 4096x4096, B = 16 encode decoded as it is, grey
(fic_decode_gray_run[_zoom]) and colour (fic_decode_rgb_run[_zoom]).  Both move the same bytes per iteration.  Wall time of
the whole call (stream upload, the device loop, the copy of the decoded image to the host), several repetitions after a warm
call; one JSON line.  Kernel times come from a separate run of this script under rocprofv3 --kernel-trace --stats.

  python tools/zoom_timing.py [--tree DIR --label NAME] [--reps N] [grey_native] [grey_zoom] [rgb_native] [rgb_zoom]

--tree DIR times the library of another checkout (the parent commit, which has the native entries only)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default="this tree")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("modes", nargs="*")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))
import fic_amd  # noqa: E402
from fic_amd import capi  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
B, WK = 16, 8


def grey_image(zoomed):
    g = np.tile(np.load(os.path.join(GOLDEN, "lena_grey_256.npy")), (4, 4))                 # 1024 x 1024
    return np.ascontiguousarray(np.kron(g, np.ones((4, 4), np.uint8))) if zoomed else np.ascontiguousarray(g)


def colour_argb(zoomed):
    rgb = np.tile(np.load(os.path.join(GOLDEN, "lena_colored_256.npy")), (4, 4, 1))
    if zoomed:
        rgb = np.kron(rgb, np.ones((4, 4, 1), np.uint8))
    c = np.ascontiguousarray(rgb).astype(np.uint32)
    return (0xFF000000 | (c[..., 0] << 16) | (c[..., 1] << 8) | c[..., 2]).astype(np.uint32).view(np.int32).reshape(-1), rgb.shape[0]


def grey_run(zoomed):
    g = grey_image(zoomed)
    return fic_amd.write_run_gray(capi.encode_gray_oneshot(g, B, WK)["qrows"], g.shape[1], g.shape[0], B, WK)


def rgb_run(zoomed):
    argb, n = colour_argb(zoomed)
    return fic_amd.write_run_rgb(capi.encode_rgb(argb, n, n, B, WK)["qrows"], n, n, B, WK)


def timed(fn):
    r = fn()                                  # warm: arena, code objects
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        r = fn()                              # the call returns after the copy of the image to the host: synchronous
        ts.append((time.perf_counter() - t0) * 1e3)
    it = int(r[2])
    return {"ms": [round(t, 3) for t in ts], "ms_median": round(float(np.median(ts)), 3), "ms_min": round(min(ts), 3),
            "iterations": it, "ms_per_iteration_median": round(float(np.median(ts)) / it, 4), "pixels": int(r[0].size)}


MODES = {
    "grey_native": lambda: (lambda run: timed(lambda: fic_amd.decode_gray_run(run)))(grey_run(True)),
    "grey_zoom": lambda: (lambda run: timed(lambda: fic_amd.decode_gray_run(run, zoom=4)))(grey_run(False)),
    "rgb_native": lambda: (lambda run: timed(lambda: fic_amd.decode_rgb_run(run)))(rgb_run(True)),
    "rgb_zoom": lambda: (lambda run: timed(lambda: fic_amd.decode_rgb_run(run, zoom=4)))(rgb_run(False)),
}
out = {"tree": args.label, "version": capi.lib().fic_version().decode()}
for m in (args.modes or list(MODES)):
    out[m] = MODES[m]()
print(json.dumps(out))
