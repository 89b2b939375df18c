#!/usr/bin/env python3
"""The batched quadtree handle (fic_amd.QuadtreeEncoder) against the one-shot entry in a loop, in one run
on one machine with warm caches.  Never bench.py's `value`.

Workload: 64 grey images of 512x512 (LenaGrey enlarged, every plane shifted differently), 16 -> 4, full search, 1 isometry,
rate-distortion pruning to at most a quarter of the 16384 smallest blocks; and the colour twin, 16 images of 512x512.
  (a) the one-shot entry called once per host image: what a caller had before the handle
  (b) the handle with host input: the upload, the encode and fic_qt_ctx_get_results_host
  (c) the handle on a device tensor: from the encode call to the end of sync
The three alternate rep by rep, so that a drift of the clock reaches all alike, and the medians are taken twice over ("run1",
"run2"): the distance between the two runs of one variant is the spread a ratio has to be read against.  Before any timing
every plane of (b) and (c) is compared with (a): leaf count, rows, lambda, statistics.

  quadtree_batch_timing.py [out.json]                 the timing
  quadtree_batch_timing.py --trace-loop N             N encodes of (c), grey then colour, and nothing else: the program to put
                                                      behind `rocprofv3 --kernel-trace --stats ... --`, in a run of its own
  quadtree_batch_timing.py --shares kernel_stats.csv [out.json]
                                                      the share of the level sweeps and of the quadtree layer in that trace,
                                                      merged into out.json when it is given"""
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, B_MAX, B_MIN = 512, 16, 4
M_LEAVES = (W // B_MIN) ** 2 // 4
QT_LAYER = ("k_leaf_sse", "k_qt_")            # the kernels of the quadtree layer; every other kernel belongs to the level encodes


def images(colour, planes):
    from fic_amd import synth
    if not colour:
        lena = np.load(os.path.join(ROOT, "tests", "golden", "lena_grey_256.npy"))
        return np.stack([synth.enlarge(lena, W, W, 3 * p, 5 * p) for p in range(planes)])
    lena = np.load(os.path.join(ROOT, "tests", "golden", "lena_colored_256.npy"))
    out = []
    for p in range(planes):
        r, g, b = (synth.enlarge(np.ascontiguousarray(lena[..., c]), W, W, 3 * p, 5 * p).astype(np.uint32) for c in range(3))
        out.append((np.uint32(0xFF000000) | (r << 16) | (g << 8) | b).view(np.int32))
    return np.stack(out)


def oneshot(fic_amd, colour, img):
    if colour:
        return fic_amd.encode_rgb_quadtree_iso_rd(img.reshape(-1), W, W, B_MAX, B_MIN, 0, 1, max_leaves=M_LEAVES)
    return fic_amd.encode_gray_quadtree_rd(img, B_MAX, B_MIN, 0, 1, max_leaves=M_LEAVES)


def ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def workload(fic_amd, colour, planes, reps):
    import torch
    imgs = images(colour, planes)
    dev = torch.from_numpy(imgs).cuda()
    torch.cuda.synchronize()
    with fic_amd.QuadtreeEncoder(W, W, B_MAX, B_MIN, 0, 1, planes, colour) as host_enc, \
            fic_amd.QuadtreeEncoder(W, W, B_MAX, B_MIN, 0, 1, planes, colour) as dev_enc:
        set_in = (lambda e, x: e.set_argb(x)) if colour else (lambda e, x: e.set_gray(x))
        set_in(dev_enc, dev)

        def a():
            return [oneshot(fic_amd, colour, imgs[p]) for p in range(planes)]

        def b():
            set_in(host_enc, imgs)
            host_enc.encode(max_leaves=M_LEAVES)
            return host_enc.results_host()

        def c():
            dev_enc.encode(max_leaves=M_LEAVES)
            dev_enc.sync()

        for _ in range(2):                                      # code objects, working sets, first-touch pages
            want = a()
            b()
            c()
        for enc in (host_enc, dev_enc):                         # faster and different is not faster
            got = enc.results()
            for p in range(planes):
                assert got[p][0].shape == want[p][0].shape and (got[p][0] == want[p][0]).all() and got[p][1] == want[p][1] \
                    and (got[p][2] == want[p][2]).all(), f"plane {p} differs from the one-shot entry"
        row = {"workload": f"{planes} x {W}x{W} {'colour' if colour else 'grey'}, {B_MAX}->{B_MIN}, n_iso 1, RD max_leaves {M_LEAVES}", "planes": planes,
               "reps": reps, "leaves": [int(len(x[0])) for x in want][:4], "equal_to_oneshot": True}
        for run in (1, 2):
            t = {"a": [], "b": [], "c": []}
            for _ in range(reps):
                t["a"].append(ms(a))
                t["b"].append(ms(b))
                t["c"].append(ms(c))
            for k, name in (("a", "a_oneshot_loop_ms"), ("b", "b_handle_host_ms"), ("c", "c_handle_device_ms")):
                row[f"{name}_run{run}"] = float(np.median(t[k]))
        for name in ("a_oneshot_loop_ms", "b_handle_host_ms", "c_handle_device_ms"):
            row[name] = (row[name + "_run1"] + row[name + "_run2"]) / 2
            row[name.replace("_ms", "_spread")] = abs(row[name + "_run1"] - row[name + "_run2"]) / min(row[name + "_run1"], row[name + "_run2"])
        row["a_over_b"] = row["a_oneshot_loop_ms"] / row["b_handle_host_ms"]
        row["a_over_c"] = row["a_oneshot_loop_ms"] / row["c_handle_device_ms"]
        return row


def trace_loop(fic_amd, n):
    import torch
    for colour, planes in ((False, 64), (True, 16)):
        dev = torch.from_numpy(images(colour, planes)).cuda()
        torch.cuda.synchronize()
        with fic_amd.QuadtreeEncoder(W, W, B_MAX, B_MIN, 0, 1, planes, colour) as enc:
            (enc.set_argb if colour else enc.set_gray)(dev)
            for _ in range(n):
                enc.encode(max_leaves=M_LEAVES)
                enc.sync()


def shares(path):
    """{"quadtree_layer_share", "level_encodes_share", "kernels": [...]} of a rocprofv3 kernel_stats.csv"""
    with open(path, newline="") as fh:
        rows = list(csv.DictReader(fh))
    name_col = next(k for k in rows[0] if k.lower() == "name")
    dur_col = next(k for k in rows[0] if "total" in k.lower() and "duration" in k.lower())
    calls_col = next(k for k in rows[0] if k.lower() == "calls")
    tot = {True: 0.0, False: 0.0}
    kernels = []
    for r in rows:
        qt = any(s in r[name_col] for s in QT_LAYER)
        tot[qt] += float(r[dur_col])
        kernels.append({"kernel": r[name_col].split("(")[0][:90], "calls": int(r[calls_col]), "total_ns": float(r[dur_col]), "quadtree_layer": qt})
    kernels.sort(key=lambda k: -k["total_ns"])
    both = tot[True] + tot[False]
    return {"quadtree_layer_share": tot[True] / both, "level_encodes_share": tot[False] / both, "kernel_ns_total": both, "kernels": kernels[:16]}


def main(argv):
    sys.path.insert(0, ROOT)
    if argv and argv[0] == "--shares":
        out = shares(argv[1])
        print(json.dumps({k: v for k, v in out.items() if k != "kernels"}))
        if len(argv) > 2:
            doc = json.load(open(argv[2])) if os.path.exists(argv[2]) else {}
            doc["kernel_trace_of_c"] = out
            json.dump(doc, open(argv[2], "w"), indent=1)
        return
    import torch                                                # before the library: its HIP runtime comes up first
    import fic_amd
    if not torch.cuda.is_available():
        raise SystemExit("quadtree_batch_timing.py needs the GPU: nothing is measured without one")
    if argv and argv[0] == "--trace-loop":
        return trace_loop(fic_amd, int(argv[1]))
    doc = {"version": fic_amd.capi.lib().fic_version().decode(),
           "rows": [workload(fic_amd, False, 64, 10), workload(fic_amd, True, 16, 10)]}
    print(json.dumps(doc, indent=1), flush=True)
    if argv:
        os.makedirs(os.path.dirname(os.path.abspath(argv[0])), exist_ok=True)
        with open(argv[0], "w") as fh:
            json.dump(doc, fh, indent=1)


if __name__ == "__main__":
    main(sys.argv[1:])
