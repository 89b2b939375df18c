"""Timing of the joint-RGB encode with 1 and 8 isometries on LenaColored tiled to a square, B = 8, full
search: a context is created, the image set once, one warm encode, then timed encodes (fic_rgb_ctx_encode + fic_rgb_ctx_sync:
everything device resident, no collage).  Every measurement is a fresh process; a round runs the parent commit's library and
this one alternately on the n_iso = 1 encode (the parent's spread against itself is the yardstick for "unchanged"), then the
n_iso = 8 encode of this tree at every size with the VALU sweep forced ("sweep" = 1) and with the matrix-core sweep forced
("sweep" = 2).  One JSON line per process.

  python tools/rgb_iso_timing.py [--parent DIR] [--rounds 3] [--reps 5] [--sizes 1024 512 256] [--out FILE]

--parent DIR: a built checkout of the parent commit (it has the n_iso = 1 entries only).  Without it only this tree runs."""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--parent", default=None)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--sizes", type=int, nargs="*", default=[1024, 512, 256])
ap.add_argument("--out", default=None)
ap.add_argument("--child", nargs=5, metavar=("TREE", "LABEL", "SIZE", "N_ISO", "SWEEP"), default=None)
args = ap.parse_args()
B = 8


def child(tree, label, size, n_iso, sweep):
    sys.path.insert(0, os.path.abspath(tree))
    import numpy as np
    import fic_amd
    from fic_amd import capi
    rgb = np.load(os.path.join(HERE, "tests", "golden", "lena_colored_256.npy"))
    rgb = np.ascontiguousarray(np.tile(rgb, (size // 256, size // 256, 1))).astype(np.uint32)
    argb = (0xFF000000 | (rgb[..., 0] << 16) | (rgb[..., 1] << 8) | rgb[..., 2]).astype(np.uint32).view(np.int32).reshape(-1)
    Dw = fic_amd.geometry(size, size, B)[2]
    kw = {"n_iso": n_iso} if n_iso != 1 else {}              # the parent's RgbEncoder has no such argument
    with capi.RgbEncoder(size, size, B, Dw, **kw) as enc:
        if sweep:
            enc.set_option("sweep", sweep)
        enc.set_argb(argb)
        enc.encode()
        enc.sync()                                            # warm: code objects, working set
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            enc.encode()
            enc.sync()
            ts.append((time.perf_counter() - t0) * 1e3)
        kernel = enc.last_kernel()
        r = enc.results()
    iso = r.get("iso")
    print(json.dumps({"tree": label, "size": size, "B": B, "n_iso": n_iso, "sweep": sweep, "kernel": kernel, "ms": [round(t, 3) for t in ts],
                      "ms_median": round(float(np.median(ts)), 3), "ms_min": round(min(ts), 3),
                      "pairs": int(r["idx_local"].size) * Dw * Dw * n_iso,
                      "iso_histogram": None if iso is None else np.bincount(iso.reshape(-1), minlength=8).tolist()}))


def run(tree, label, size, n_iso, sweep, sink):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--child", tree, label, str(size), str(n_iso), str(sweep)],
                       capture_output=True, text=True, timeout=300)
    line = p.stdout.strip().splitlines()[-1] if p.returncode == 0 and p.stdout.strip() else json.dumps(
        {"tree": label, "size": size, "n_iso": n_iso, "error": p.returncode, "stderr": p.stderr[-400:]})
    print(line, flush=True)
    if sink:
        sink.write(line + "\n")
        sink.flush()
    return p.returncode


if args.child:
    child(args.child[0], args.child[1], int(args.child[2]), int(args.child[3]), int(args.child[4]))
else:
    sink = open(args.out, "w") if args.out else None
    rc = 0
    for rnd in range(args.rounds):
        big = max(args.sizes)
        for tree, label in (([(args.parent, "parent")] if args.parent else []) + [(HERE, "this")]) * 2:
            rc = rc or run(tree, f"{label} (round {rnd})", big, 1, 0, sink)
            if rc:                                            # a failed GPU process: start nothing more
                sys.exit(rc)
        for size in args.sizes:
            for sweep in (1, 2):
                rc = rc or run(HERE, f"this (round {rnd})", size, 8, sweep, sink)
                if rc:
                    sys.exit(rc)
    sys.exit(rc)
