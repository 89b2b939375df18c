#!/usr/bin/env python3
"""Timings of the least-squares domain search (option "search" = 1) beside the reference criterion's
sweeps on the same context geometry: LenaGrey enlarged to 512x512 (B = 8) and 1024x1024 (B = 4), full search, 1 and 8
isometries, one image resident on the device.  Per setting four contexts -- least squares on the VALU (k_sweep_lsq_fast), least
squares on the matrix cores ("lsq_engine" = 1, k_sweep_lsq_q), the reference criterion through the VALU
sweep k_sweep_fast ("sweep" = 2) and through the default sweep ("sweep" = 0) -- are warmed up and then timed in alternation: the
host clock around encode + sync (the whole encode: prep, sweep, finalise) and the sweep kernel alone from the "time_sweep"
events.  Medians of `reps` rounds.  After the timed rounds one more encode of each least-squares context runs under
"sweep_stats": pairs evaluated exactly per range block and the share of (wave, pool block) visits / tiles that had some.  With
--check the codebooks of both least-squares sweeps are also compared with the generic sweep's at these sizes.  With
--chunk-sweep a,b,.. the matrix-core sweep is also timed (sweep kernel, `reps` encodes each) under "chunks" = a, b, ..; 0 is the
automatic count.  Never bench.py's `value`.

Usage: lsq_timing.py [out.json] [--reps N] [--check] [--chunk-sweep 1,2,4,8]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(argv):
    out_path, reps, check, chunk_sweep = None, 15, False, []
    it = iter(argv)
    for a in it:
        if a == "--reps":
            reps = int(next(it))
        elif a == "--check":
            check = True
        elif a == "--chunk-sweep":
            chunk_sweep = [int(x) for x in next(it).split(",")]
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
            for name, opts in (("lsq", {"search": 1}), ("lsq_q", {"search": 1, "lsq_engine": 1}), ("reference_sweep2", {"sweep": 2}),
                               ("reference_default", {})):
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
            row["lsq_q"]["sweep_ratio_to_lsq"] = round(row["lsq_q"]["sweep_ms_mean"] / row["lsq"]["sweep_ms_mean"], 4)
            row["lsq_q"]["encode_ratio_to_lsq"] = round(row["lsq_q"]["encode_ms_median"] / row["lsq"]["encode_ms_median"], 4)
            for name in ("lsq", "lsq_q"):                       # the counters, outside the timed rounds
                enc = encs[name]
                enc.set_option("sweep_stats", 1)
                enc.encode()
                st = enc.sweep_stats()
                enc.set_option("sweep_stats", 0)
                row[name]["exact_pairs_per_range"] = round(st["exact_pairs"] / enc.n_ranges, 2)
                row[name]["exact_pair_share"] = round(st["exact_pairs"] / (enc.n_ranges * enc.n_domains * n_iso), 6)
                row[name]["flagged_share"] = round(st["flagged_tiles"] / max(st["tiles"], 1), 4)
            if chunk_sweep:
                enc = encs["lsq_q"]
                row["lsq_q_chunk_sweep"] = {}
                for c in chunk_sweep:
                    enc.set_option("chunks", c)
                    enc.encode()
                    enc.sync()
                    enc.sweep_time(reset=True)
                    for _ in range(reps):
                        enc.encode()
                    ms, n = enc.sweep_time(reset=True)
                    row["lsq_q_chunk_sweep"][str(c)] = {"chunks": enc.info()["chunks"], "sweep_ms_mean": round(ms / max(n, 1), 4)}
                enc.set_option("chunks", 0)
            if check:
                enc = encs["lsq"]
                fast = dict(enc.results(), E=enc.lsq_error())
                encs["lsq_q"].encode()
                mfma = dict(encs["lsq_q"].results(), E=encs["lsq_q"].lsq_error())
                enc.set_option("sweep", 1)
                enc.encode()
                slow = dict(enc.results(), E=enc.lsq_error())
                row["fast_equals_generic"] = bool(all((fast[k].view(np.uint8) == slow[k].view(np.uint8)).all() for k in fast))
                row["lsq_q_equals_generic"] = bool(all((mfma[k].view(np.uint8) == slow[k].view(np.uint8)).all() for k in mfma))
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
