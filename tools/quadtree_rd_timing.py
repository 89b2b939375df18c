#!/usr/bin/env python3
"""The quadtree encode by rate-distortion pruning against the encode to a leaf budget by threshold
(section 4.18), through their C entry points (host buffers in and out, warm caches).  Never bench.py's `value`.

Timing: LenaGrey enlarged to 512x512 and 2048x2048, 16 -> 4, full search, 1 isometry, the budget = the leaf count of threshold
400 (the geometries of tools/quadtree_budget_timing.py).  The two encodes alternate call by call, so that a drift of the clock
reaches both alike; the medians of `reps` calls are taken twice over ("run 1", "run 2"): the distance between the two runs of
one entry is the spread that a difference between the entries has to be read against.

Decoded PSNR: LenaGrey 256x256, 16 -> 4, the budgets 259 .. 4095, both search criteria: the tree of the pruning and the tree
of the threshold rule with at most that many leaves, each written as a tag-2 stream, decoded at zoom 1 and compared with the
original.  The budget entries take the reference criterion only; under least squares the threshold is found from outside, by
bisection over the float32 thresholds of the fixed-threshold entry (the smallest whose tree fits).

Usage: quadtree_rd_timing.py [out.txt] [--no-timing] [--no-psnr]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGETS = (259, 512, 1024, 2048, 4095)


def ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def psnr(a, b):
    mse = float(((a.astype(np.float64) - b.astype(np.float64)) ** 2).mean())
    return float("inf") if mse == 0 else 10.0 * np.log10(255.0 * 255.0 / mse)


def threshold_for_budget(fic_amd, g, M, search):
    """The smallest non-negative float32 threshold whose tree has at most M leaves, by bisection over the bit patterns."""
    lo, hi = 0, int(np.float32(np.inf).view(np.uint32))             # the tree at +inf always fits
    leaves = lambda bits: len(fic_amd.encode_gray_quadtree(g, 16, 4, 0, 1, float(np.uint32(bits).view(np.float32)), search=search))   # noqa: E731
    if leaves(lo) <= M:
        return np.float32(0.0)
    while hi - lo > 1:                                              # leaves(lo) > M >= leaves(hi)
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if leaves(mid) <= M else (mid, hi)
    return np.uint32(hi).view(np.float32)


def timing(fic_amd, lena):
    from fic_amd import synth
    rows = []
    for W, reps in ((512, 20), (2048, 10)):
        g = synth.enlarge(lena, W, W)
        M = len(fic_amd.encode_gray_quadtree(g, 16, 4, 0, 1, 400.0))
        rd = lambda: fic_amd.encode_gray_quadtree_rd(g, 16, 4, 0, 1, max_leaves=M)            # noqa: E731
        budget = lambda: fic_amd.encode_gray_quadtree_budget(g, 16, 4, 0, 1, max_leaves=M)    # noqa: E731
        for _ in range(2):                                          # code objects, working sets, first-touch pages
            (leaves, lam, stats), (bleaves, t, bstats) = rd(), budget()
        assert len(leaves) <= M and len(bleaves) <= M
        r = {"image": f"{W}x{W}", "max_leaves": M, "reps": reps,
             "rd": {"lambda": lam, "leaves": int(len(leaves)), "collage_sse": int(stats[0])},
             "threshold": {"threshold": float(t), "leaves": int(len(bleaves)), "collage_sse": int(bstats[0])}}
        for run in (1, 2):
            a, b = [], []
            for _ in range(reps):
                a.append(ms(rd))
                b.append(ms(budget))
            r[f"rd_ms_run{run}"], r[f"threshold_ms_run{run}"] = float(np.median(a)), float(np.median(b))
        r["rd_over_threshold"] = (r["rd_ms_run1"] + r["rd_ms_run2"]) / (r["threshold_ms_run1"] + r["threshold_ms_run2"])
        r["spread_rd"] = abs(r["rd_ms_run1"] - r["rd_ms_run2"]) / min(r["rd_ms_run1"], r["rd_ms_run2"])
        r["spread_threshold"] = abs(r["threshold_ms_run1"] - r["threshold_ms_run2"]) / min(r["threshold_ms_run1"], r["threshold_ms_run2"])
        rows.append(r)
    return rows


def decoded_psnr(fic_amd, lena):
    rows = []

    def decoded(leaves):
        return psnr(fic_amd.decode_quadtree_run(fic_amd.write_run_quadtree(leaves, 256, 256, 16, 4, 0, 1))[0], lena)

    for search in ("reference", "lsq"):
        for M in BUDGETS:
            leaves, lam, stats = fic_amd.encode_gray_quadtree_rd(lena, 16, 4, 0, 1, search=search, max_leaves=M)
            if search == "reference":
                bleaves, t, bstats = fic_amd.encode_gray_quadtree_budget(lena, 16, 4, 0, 1, max_leaves=M)
                b_sse = int(bstats[0])
            else:
                t = threshold_for_budget(fic_amd, lena, M, search)
                bleaves = fic_amd.encode_gray_quadtree(lena, 16, 4, 0, 1, float(t), search=search)
                b_sse = None                                        # no SSE hook under least squares
            assert len(leaves) <= M and len(bleaves) <= M
            rows.append({"image": "lena_grey_256", "search": search, "max_leaves": M,
                         "rd": {"lambda": lam, "leaves": int(len(leaves)), "collage_sse": int(stats[0]), "decoded_psnr_db": decoded(leaves)},
                         "threshold": {"threshold": float(t), "leaves": int(len(bleaves)), "collage_sse": b_sse, "decoded_psnr_db": decoded(bleaves)}})
            rows[-1]["decoded_gain_db"] = rows[-1]["rd"]["decoded_psnr_db"] - rows[-1]["threshold"]["decoded_psnr_db"]
            if b_sse:
                rows[-1]["collage_gain_db"] = 10.0 * np.log10(b_sse / int(stats[0]))
    return rows


def main(argv):
    out_path = next((a for a in argv if not a.startswith("--")), None)
    sys.path.insert(0, ROOT)
    import fic_amd
    lena = np.load(os.path.join(ROOT, "tests", "golden", "lena_grey_256.npy"))
    rows = []
    if "--no-timing" not in argv:
        rows += timing(fic_amd, lena)
    if "--no-psnr" not in argv:
        rows += decoded_psnr(fic_amd, lena)
    lines = [json.dumps(r) for r in rows]
    print("\n".join(lines), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
