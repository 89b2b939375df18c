#!/usr/bin/env python3
"""Timings of the least-squares domain search (option "search" = 1) beside the reference criterion's
sweeps on the same context geometry: LenaGrey enlarged to 512x512 (B = 8) and 1024x1024 (B = 4), full search, 1 and 8
isometries, one image resident on the device.  Per setting three contexts -- least squares (k_sweep_lsq_fast), the reference
criterion through the VALU sweep k_sweep_fast ("sweep" = 2) and through the default sweep ("sweep" = 0) -- are warmed up and
then timed in alternation: the host clock around encode + sync (the whole encode: prep, sweep, finalise) and the sweep kernel
alone from the "time_sweep" events.  Medians of `reps` rounds.  With --check the least-squares codebook of the fast sweep is
also compared with the generic sweep's at these sizes.  Never bench.py's `value`.

Usage: lsq_timing.py [out.json] [--reps N] [--check]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(argv):
    out_path, reps, check = None, 15, False
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
    lena = np.load(os.path.join(ROOT, "tests", "golden", "lena_grey_256.npy"))
    rows = []
    for W, B in ((512, 8), (1024, 4)):
        g = synth.enlarge(lena, W, W)
        for n_iso in (1, 8):
            encs = {}
            for name, opts in (("lsq", {"search": 1}), ("reference_sweep2", {"sweep": 2}), ("reference_default", {})):
                enc = fic_amd.Encoder(W, W, B, None, n_iso)
                for k, v in opts.items():
                    enc.set_option(k, v)
                enc.set_option("time_sweep", 1)
                enc.set_gray(g)
                for _ in range(3):                              # code objects, working sets
                    enc.encode()
                    enc.sync()
                enc.sweep_time(reset=True)
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
                ms, n = enc.sweep_time(reset=True)
                row[name] = {"encode_ms_median": round(float(np.median(wall[name])), 4), "encode_ms_min": round(min(wall[name]), 4),
                             "sweep_ms_mean": round(ms / max(n, 1), 4), "kernel": enc.last_kernel(), "chunks": enc.info()["chunks"]}
            if check:
                enc = encs["lsq"]
                fast = dict(enc.results(), E=enc.lsq_error())
                enc.set_option("sweep", 1)
                enc.encode()
                slow = dict(enc.results(), E=enc.lsq_error())
                row["fast_equals_generic"] = bool(all((fast[k].view(np.uint8) == slow[k].view(np.uint8)).all() for k in fast))
                qa = fast["qrows"][0, :, 1]
                row["rows_clamped"] = round(float((np.abs(qa) == 100).mean()), 4)
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
