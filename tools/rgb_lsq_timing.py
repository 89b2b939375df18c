#!/usr/bin/env python3
"""Timings of the least-squares domain search of the joint-RGB path (option "search" = 1 of a colour context, DESIGN.md sections
4.20 and 4.22): LenaColored enlarged to 512x512 and 1024x1024 (channel by channel), B = 4, 8 and 16, full search, 1 and 8
isometries, one image resident on the device.  Per setting three contexts are warmed up and then timed in alternating rounds
within this one run:
  lsq_q              least squares on the matrix cores ("lsq_engine" = 1, k_sweep_lsq_rgb_q),
  lsq                its VALU twin ("lsq_engine" = 0: k_sweep_lsq_rgb_fast at B <= 8, k_sweep_lsq_rgb_generic at B = 16),
  reference_default  the reference criterion through its default sweep ("sweep" = 0).
Reported per context: the host clock around encode + sync (the whole encode: scale, prep, sweep, finalise; median of the rounds)
and, for the two least-squares contexts, the sweep kernel alone from the "time_sweep" events (mean, and the smallest and largest
round).  The twin is the yardstick: lsq_q counts as ahead only where its mean sweep time lies below the twin's by more than the
spread (largest minus smallest round) of the twin's own rounds in this run.  After the timing, outside the timed rounds: the
"sweep_stats" counters of both sweeps, with --chunks a sweep over the option "chunks" of lsq_q, and with --check the codebooks of
the two engines compared byte for byte.  Never bench.py's `value`.

Usage: rgb_lsq_timing.py [out.json] [--reps N] [--check] [--chunks] [--sizes 512,1024] [--blocks 4,8,16]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK_COUNTS = (1, 2, 4, 8, 16, 32, 64)


def timed_sweep(enc, reps):
    enc.sweep_time()
    for _ in range(reps):
        enc.encode()
    enc.sync()
    ms, n = enc.sweep_time()
    return ms / max(n, 1)


def main(argv):
    out_path, reps, check, chunk_sweep, sizes, blocks = None, 7, False, False, (512, 1024), (4, 8, 16)
    it = iter(argv)
    for a in it:
        if a == "--reps":
            reps = int(next(it))
        elif a == "--check":
            check = True
        elif a == "--chunks":
            chunk_sweep = True
        elif a == "--sizes":
            sizes = tuple(int(x) for x in next(it).split(","))
        elif a == "--blocks":
            blocks = tuple(int(x) for x in next(it).split(","))
        else:
            out_path = a
    sys.path.insert(0, ROOT)
    import fic_amd
    from fic_amd import capi, synth
    lena = np.load(os.path.join(ROOT, "tests", "golden", "lena_colored_256.npy"))
    rows = []
    for W in sizes:
        rgb = np.stack([synth.enlarge(np.ascontiguousarray(lena[..., ch]), W, W) for ch in range(3)], axis=-1).astype(np.uint32)
        argb = (0xFF000000 | (rgb[..., 0] << 16) | (rgb[..., 1] << 8) | rgb[..., 2]).astype(np.uint32).view(np.int32).reshape(-1)
        for B in blocks:
            wK = fic_amd.geometry(W, W, B)[2]
            for n_iso in (1, 8):
                encs = {}
                for name, opts in (("lsq_q", {"search": 1, "lsq_engine": 1}), ("lsq", {"search": 1}), ("reference_default", {})):
                    enc = capi.RgbEncoder(W, W, B, wK, n_iso=n_iso)
                    for k, v in opts.items():
                        enc.set_option(k, v)
                    if "search" in opts:
                        enc.set_option("time_sweep", 1)
                    enc.set_argb(argb)
                    for _ in range(2):                          # code objects, working sets
                        enc.encode()
                        enc.sync()
                    if "search" in opts:
                        enc.sweep_time()
                    encs[name] = enc
                wall, sweep = {k: [] for k in encs}, {k: [] for k in encs}
                for _ in range(reps):
                    for name, enc in encs.items():
                        t0 = time.perf_counter()
                        enc.encode()
                        enc.sync()
                        wall[name].append((time.perf_counter() - t0) * 1e3)
                        if name != "reference_default":
                            sweep[name].append(enc.sweep_time()[0])
                row = {"W": W, "B": B, "n_iso": n_iso, "reps": reps}
                for name, enc in encs.items():
                    row[name] = {"encode_ms_median": round(float(np.median(wall[name])), 4), "encode_ms_min": round(min(wall[name]), 4),
                                 "kernel": enc.last_kernel()}
                    if sweep[name]:
                        row[name].update(sweep_ms_mean=round(float(np.mean(sweep[name])), 4), sweep_ms_min=round(min(sweep[name]), 4),
                                         sweep_ms_max=round(max(sweep[name]), 4), chunks=enc.last_lsq_chunks())
                q, twin = row["lsq_q"], row["lsq"]
                q["sweep_ratio_to_lsq"] = round(q["sweep_ms_mean"] / twin["sweep_ms_mean"], 4)
                q["encode_ratio_to_lsq"] = round(q["encode_ms_median"] / twin["encode_ms_median"], 4)
                twin["sweep_ms_spread"] = round(twin["sweep_ms_max"] - twin["sweep_ms_min"], 4)
                q["ahead_of_lsq"] = bool(q["sweep_ms_mean"] < twin["sweep_ms_mean"] - twin["sweep_ms_spread"])
                pairs = int(encs["lsq"].n_ranges) * wK * wK * n_iso
                for name in ("lsq", "lsq_q"):                       # the counters, outside the timed rounds
                    enc = encs[name]
                    enc.set_option("sweep_stats", 1)
                    enc.encode()
                    st = enc.sweep_stats()
                    enc.set_option("sweep_stats", 0)
                    # lsq_q: tile epilogues (32 x 32 pairs), tiles with flagged pairs; lsq (fast): (wave, pool block) visits, visits with the epilogue
                    row[name]["stats"] = {"tiles": st["tiles"], "flagged_tiles": st["flagged_tiles"], "exact_pairs": st["exact_pairs"],
                                          "waves": st["waves"], "pairs": pairs,
                                          "exact_pairs_per_range_block": round(st["exact_pairs"] / int(enc.n_ranges), 2)}
                if check:
                    enc = encs["lsq"]
                    enc.encode()
                    valu = dict(enc.results(), E=enc.lsq_error())
                    enc = encs["lsq_q"]
                    enc.encode()
                    mfma = dict(enc.results(), E=enc.lsq_error())
                    row["lsq_q_equals_lsq"] = bool(all((mfma[k].view(np.uint8) == valu[k].view(np.uint8)).all() for k in mfma))
                if chunk_sweep:
                    enc = encs["lsq_q"]
                    row["lsq_q_chunk_sweep"] = {}
                    seen = set()
                    for c in CHUNK_COUNTS:
                        enc.set_option("chunks", c)
                        enc.encode()
                        enc.sync()
                        got = enc.last_lsq_chunks()
                        if got in seen:
                            continue
                        seen.add(got)
                        row["lsq_q_chunk_sweep"][str(c)] = {"chunks": got, "sweep_ms_mean": round(timed_sweep(enc, max(3, reps // 2)), 4)}
                    enc.set_option("chunks", 0)
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
