#!/usr/bin/env python3
"""Decoding a batch from the quadtree handle (fic_amd.QuadtreeEncoder.decode) against what a caller had
before it, in one run on one machine with warm caches.  Never bench.py's `value`.

Workloads: those of tools/quadtree_batch_timing.py -- 64 grey images of 512x512 (LenaGrey enlarged, every plane shifted
differently) and 16 colour ones, 16 -> 4, full search, 1 isometry, rate-distortion pruning to at most 4096 leaves -- encoded once
on a device tensor; then, at zoom 1 and 2,
  (a) write_runs() and the one-shot decoder of the context's format once per plane
  (b) decode(zoom): every plane at once, from the tables on the device
The two alternate rep by rep, so that a drift of the clock reaches both alike, and the medians of 10 are taken twice over
("run1", "run2"): the distance between the two runs of one variant is the spread a ratio has to be read against.  Before any
timing every plane of (b) is compared with (a): image, avgError bits, iterations.

  quadtree_batch_decode_timing.py [out.json]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from quadtree_batch_timing import B_MAX, B_MIN, M_LEAVES, W, images, ms  # noqa: E402


def workload(fic_amd, colour, planes, zoom, reps):
    import torch
    capi = fic_amd.capi
    dev = torch.from_numpy(images(colour, planes)).cuda()
    torch.cuda.synchronize()
    oneshot = capi.decode_rgb_quadtree_iso_run if colour else capi.decode_quadtree_run
    with fic_amd.QuadtreeEncoder(W, W, B_MAX, B_MIN, 0, 1, planes, colour) as enc:
        (enc.set_argb if colour else enc.set_gray)(dev)
        enc.encode(max_leaves=M_LEAVES)
        enc.sync()

        def a():
            return [oneshot(run, zoom=zoom) for run in enc.write_runs()]

        def b():
            return enc.decode(zoom=zoom)

        for _ in range(2):                                      # code objects, arenas, first-touch pages
            want = a()
            got = b()
        for p in range(planes):                                 # faster and different is not faster
            assert (got[0][p] == want[p][0]).all() and np.float32(got[1][p]).view(np.uint32) == np.float32(want[p][1]).view(np.uint32) \
                and int(got[2][p]) == int(want[p][2]), f"plane {p} differs from the one-shot decoder"
        row = {"workload": f"{planes} x {W}x{W} {'colour' if colour else 'grey'}, {B_MAX}->{B_MIN}, n_iso 1, RD max_leaves {M_LEAVES}, zoom {zoom}",
               "planes": planes, "zoom": zoom, "reps": reps, "iterations": sorted({int(x) for x in got[2]}), "equal_to_oneshot": True}
        for run in (1, 2):
            t = {"a": [], "b": []}
            for _ in range(reps):
                t["a"].append(ms(a))
                t["b"].append(ms(b))
            row[f"a_runs_and_oneshot_loop_ms_run{run}"] = float(np.median(t["a"]))
            row[f"b_handle_decode_ms_run{run}"] = float(np.median(t["b"]))
        for name in ("a_runs_and_oneshot_loop_ms", "b_handle_decode_ms"):
            r1, r2 = row[name + "_run1"], row[name + "_run2"]
            row[name] = (r1 + r2) / 2
            row[name.replace("_ms", "_spread")] = abs(r1 - r2) / min(r1, r2)
        row["a_over_b"] = row["a_runs_and_oneshot_loop_ms"] / row["b_handle_decode_ms"]
        enc.collage()
        row["collage_ms"] = float(np.median([ms(enc.collage) for _ in range(reps)]))     # at the encoded size, whatever the zoom
        return row


def main(argv):
    sys.path.insert(0, ROOT)
    import torch                                                # before the library: its HIP runtime comes up first
    import fic_amd
    if not torch.cuda.is_available():
        raise SystemExit("quadtree_batch_decode_timing.py needs the GPU: nothing is measured without one")
    doc = {"version": fic_amd.capi.lib().fic_version().decode(),
           "rows": [workload(fic_amd, colour, planes, zoom, 10) for colour, planes in ((False, 64), (True, 16)) for zoom in (1, 2)]}
    print(json.dumps(doc, indent=1), flush=True)
    if argv:
        os.makedirs(os.path.dirname(os.path.abspath(argv[0])), exist_ok=True)
        with open(argv[0], "w") as fh:
            json.dump(doc, fh, indent=1)


if __name__ == "__main__":
    main(sys.argv[1:])
