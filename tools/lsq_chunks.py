#!/usr/bin/env python3
"""Pool chunk count against sweep time and survivors for the least-squares fast sweep k_sweep_lsq_fast:
LenaGrey enlarged, full search; per "chunks" value 7 timed encodes ("time_sweep"), then one encode with "sweep_stats" = 1.
One JSON line per setting: (wave, pool block) visits, the visits that ran the exact epilogue, the pairs evaluated exactly.
profiles/lsq_timing.txt part 2 is a run of this script."""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fic_amd
from fic_amd import synth
lena = np.load(os.path.join(ROOT, "tests", "golden", "lena_grey_256.npy"))
for W, B, n_iso, chunks in ((1024, 4, 1, (0, 4, 8, 16, 32)), (1024, 4, 8, (0, 4, 8, 16)), (512, 8, 1, (0, 4, 8, 16)), (512, 8, 8, (0, 4, 8, 16))):
    g = synth.enlarge(lena, W, W)
    with fic_amd.Encoder(W, W, B, None, n_iso) as enc:
        enc.set_option("search", 1)
        enc.set_option("time_sweep", 1)
        enc.set_gray(g)
        for c in chunks:
            enc.set_option("chunks", c)
            enc.set_option("sweep_stats", 0)
            for _ in range(3):
                enc.encode(); enc.sync()
            enc.sweep_time(reset=True)
            for _ in range(7):
                enc.encode(); enc.sync()
            ms, n = enc.sweep_time(reset=True)
            enc.set_option("sweep_stats", 1)
            enc.encode(); enc.sync()
            st = enc.sweep_stats()
            pairs = enc.n_ranges * enc.n_domains * n_iso
            print(json.dumps({"W": W, "B": B, "n_iso": n_iso, "chunks_opt": c, "chunks": enc.info()["chunks"], "sweep_ms": round(ms / n, 4),
                              "visits": st["tiles"], "slow_visits": st["flagged_tiles"], "slow_share": round(st["flagged_tiles"] / max(st["tiles"], 1), 4),
                              "exact_pairs": st["exact_pairs"], "survivor_rate": round(st["exact_pairs"] / pairs, 6), "waves": st["waves"]}), flush=True)
