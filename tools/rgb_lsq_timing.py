#!/usr/bin/env python3
"""Timings of the least-squares domain search of the joint-RGB path (option "search" = 1 of a colour context, DESIGN.md section
4.20) beside the reference criterion's sweeps on the same context geometry: LenaColored enlarged to 512x512 and 1024x1024
(channel by channel), B = 4 and 8, full search, 1 and 8 isometries, one image resident on the device.  Per setting three contexts
-- least squares (k_sweep_lsq_rgb_fast), the reference criterion through the VALU sweep k_sweep_rgb_fast[_iso] ("sweep" = 1) and
through the default sweep ("sweep" = 0) -- are warmed up and then timed in alternation with the host clock around encode + sync:
the whole encode (scale, prep, sweep, finalise).  A colour context has no "time_sweep" events, so the sweep alone is not timed:
every figure and ratio is an encode's, and on the smallest settings launch overhead is a visible share of it.  Medians of `reps`
rounds.  The "sweep_stats" counters of the least-squares sweep (survivors of the prune) come from one more encode after the
timing.  With --check the least-squares codebook of the fast sweep is also compared with the generic sweep's at these sizes.
Never bench.py's `value`.

Usage: rgb_lsq_timing.py [out.json] [--reps N] [--check]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(argv):
    out_path, reps, check = None, 9, False
    it = iter(argv)
    for a in it:
        if a == "--reps":
            reps = int(next(it))
        elif a == "--check":
            check = True
        else:
            out_path = a
    sys.path.insert(0, ROOT)
    import fic_amd
    from fic_amd import capi, synth
    lena = np.load(os.path.join(ROOT, "tests", "golden", "lena_colored_256.npy"))
    rows = []
    for W in (512, 1024):
        rgb = np.stack([synth.enlarge(np.ascontiguousarray(lena[..., ch]), W, W) for ch in range(3)], axis=-1).astype(np.uint32)
        argb = (0xFF000000 | (rgb[..., 0] << 16) | (rgb[..., 1] << 8) | rgb[..., 2]).astype(np.uint32).view(np.int32).reshape(-1)
        for B in (8, 4):
            wK = fic_amd.geometry(W, W, B)[2]
            for n_iso in (1, 8):
                encs = {}
                for name, opts in (("lsq", {"search": 1}), ("reference_sweep1", {"sweep": 1}), ("reference_default", {})):
                    enc = capi.RgbEncoder(W, W, B, wK, n_iso=n_iso)
                    for k, v in opts.items():
                        enc.set_option(k, v)
                    enc.set_argb(argb)
                    for _ in range(2):                          # code objects, working sets
                        enc.encode()
                        enc.sync()
                    encs[name] = enc
                wall = {k: [] for k in encs}
                for _ in range(reps):
                    for name, enc in encs.items():
                        t0 = time.perf_counter()
                        enc.encode()
                        enc.sync()
                        wall[name].append((time.perf_counter() - t0) * 1e3)
                row = {"W": W, "B": B, "n_iso": n_iso, "reps": reps}
                for name, enc in encs.items():
                    row[name] = {"encode_ms_median": round(float(np.median(wall[name])), 4), "encode_ms_min": round(min(wall[name]), 4),
                                 "kernel": enc.last_kernel()}
                row["lsq_over_reference_sweep1"] = round(row["lsq"]["encode_ms_median"] / row["reference_sweep1"]["encode_ms_median"], 3)
                row["lsq_over_reference_default"] = round(row["lsq"]["encode_ms_median"] / row["reference_default"]["encode_ms_median"], 3)
                enc = encs["lsq"]
                enc.set_option("sweep_stats", 1)
                enc.encode()
                st = enc.sweep_stats()
                enc.set_option("sweep_stats", 0)
                # the counters of k_sweep_lsq_rgb_fast: (wave, pool block) visits, visits with the exact epilogue, pairs evaluated exactly, waves
                row["lsq_stats"] = {"visits": st["tiles"], "visits_with_epilogue": st["flagged_tiles"], "exact_pairs": st["exact_pairs"],
                                    "waves": st["waves"], "pairs": int(enc.n_ranges) * wK * wK * n_iso}
                if check:
                    fast = dict(enc.results(), E=enc.lsq_error())
                    enc.set_option("sweep", 1)
                    enc.encode()
                    slow = dict(enc.results(), E=enc.lsq_error())
                    row["fast_equals_generic"] = bool(all((fast[k].view(np.uint8) == slow[k].view(np.uint8)).all() for k in fast))
                    row["rows_clamped"] = round(float((np.abs(fast["qrows"][0, :, 1]) == 1000000).mean()), 4)
                for enc in encs.values():
                    enc.close()
                rows.append(row)
                print(json.dumps(row), flush=True)
    out = {"version": capi.lib().fic_version().decode(), "rows": rows}
    if out_path:
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
