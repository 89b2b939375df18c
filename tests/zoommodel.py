"""Reference models of decoding at zoom z in {1, 2, 4}, built on the unchanged oracle: the stream of a
w x h, block-B image decoded on the geometry (z*w, z*h, z*B, wK).  Fixed-B streams: the oracle's own decoders on the stream
with the header ints {w, h, B} replaced -- the reference's decoder has no limit on the block size.  Quadtree streams: the
numpy loops of qtmodel.decode / qtrgbmodel.decode with every leaf {x, y, B} and the geometry multiplied by z (the streams are
parsed at zoom 1: the readers know the levels 16 / 8 / 4 only).  Test infrastructure only."""
import struct

import numpy as np

import qtmodel as qm
import qtrgbmodel as rm
from oracle import fic_oracle as fo


def rescale_header(run, z):
    """The fixed-B .run stream {isRGB, w, h, B, wK, rows...} with {z*w, z*h, z*B} in its header, rows unchanged."""
    tag, w, h, B, wK = struct.unpack(">5i", run[:20])
    return struct.pack(">5i", tag, z * w, z * h, z * B, wK) + bytes(run[20:])


def fixed_run(tag, rows, w, h, B, wK):
    """A fixed-B .run stream from its quantised rows (int [N_r, 3] grey, tag 0; [N_r, 5] colour, tag 1)."""
    return struct.pack(">5i", tag, w, h, B, wK) + np.ascontiguousarray(rows, ">i4").tobytes()


def decode_gray(run, z, avg_error_in=0.0):
    """(gray uint8 [z*h, z*w], avgError float32, iterations): decodeGreyScale on the header-rescaled stream."""
    return fo.decode_gray(rescale_header(run, z), avg_error_in)


def decode_rgb(run, z, avg_error_in=0.0):
    """(rgb uint8 [z*h, z*w, 3], avgError float32, iterations): decodeRGB on the header-rescaled stream."""
    return fo.decode_rgb(rescale_header(run, z), avg_error_in)


def decode_rows(qrows, iso, w, h, B, wK, z, avg_error_in=0.0):
    """The same from quantised rows + isometry ids (the n_iso = 8 extension)."""
    return fo.decode_rows(qrows, iso, z * w, z * h, z * B, wK, avg_error_in)


def _loop(w, h, per, start, scale, paint, avg_error_in):
    """The decoder loop shared by both formats over per = {B: (leaf arguments of paint..., rr, cc, sqbuf offsets)}."""
    img = start
    avg = np.float32(avg_error_in)
    iters = 0
    for counter in range(50):
        src = scale(img)                                            # the pools of the image before the paint
        vals = {B: paint(src, B, *p[:-3]) for B, p in per.items()}
        sq = np.zeros(w * h, np.int64)
        for B, p in per.items():
            rr, cc, so = p[-3:]
            d = img[rr, cc].astype(np.int64) - vals[B]
            sq[so] = d * d if d.ndim == 2 else (d * d).sum(axis=-1)
            img[rr, cc] = vals[B]
        acc = np.add.accumulate(np.concatenate([[avg], sq.astype(np.float32)]).astype(np.float32), dtype=np.float32)
        avg = np.float32(acc[-1] / np.float32(w * h))
        iters = counter + 1
        if avg < 1:
            break
        if counter != 49:
            avg = np.float32(0.0)
    return img, np.float32(avg), iters


def _zoomed_levels(hd, leaves, z):
    """Per zoomed side z*B: (leaves of that side with x, y, B multiplied by z, their global domain block, pixel rows and
    columns, offsets of their squares in stream order); the zoomed size."""
    w, h = z * hd["w"], z * hd["h"]
    lz = leaves.copy()
    lz[:, :3] *= z
    Bs = lz[:, 2].astype(np.int64)
    offs = np.concatenate([[0], np.cumsum(Bs * Bs)[:-1]])
    out = {}
    for B0 in qm.levels(hd["B_max"], hd["B_min"]):
        B = z * B0
        sel = np.nonzero(Bs == B)[0]
        if sel.size == 0:
            continue
        lv = lz[sel]
        Rw = w // B
        j = (lv[:, 1] // B) * Rw + lv[:, 0] // B
        loc = np.zeros((h // B) * Rw, np.int32)
        loc[j] = lv[:, 3]
        gi = qm.global_index(w, h, B, qm.level_wk(w, h, B, hd["wK"]), loc)[j]     # the level's own window: Dw does not change
        pos = np.arange(B * B)
        out[B] = (lv, gi, lv[:, 1][:, None] + pos // B, lv[:, 0][:, None] + pos % B, offs[sel][:, None] + pos)
    return out, w, h


def decode_quadtree(run, z, avg_error_in=0.0):
    """qtmodel.decode at zoom z: (gray uint8 [z*h, z*w], avgError float32, iterations)."""
    hd, leaves = qm.read_run(run)
    lev, w, h = _zoomed_levels(hd, leaves, z)
    per = {B: (gi, lv[:, 4], lv[:, 5], lv[:, 6], rr, cc, so) for B, (lv, gi, rr, cc, so) in lev.items()}
    return _loop(w, h, per, np.full((h, w), 128, np.uint8), lambda img: img.copy(), qm.paint_values, avg_error_in)


def decode_rgb_quadtree(run, z, avg_error_in=0.0):
    """qtrgbmodel.decode at zoom z: (rgb uint8 [z*h, z*w, 3], avgError float32, iterations)."""
    hd, leaves = rm.read_run(run)
    lev, w, h = _zoomed_levels(hd, leaves, z)
    per = {B: (gi, lv[:, 3:], rr, cc, so) for B, (lv, gi, rr, cc, so) in lev.items()}
    img, avg, it = _loop(w, h, per, np.full((h, w, 3), 128, np.int64), rm.scale_rgb, rm.paint_values, avg_error_in)
    return img.astype(np.uint8), avg, it


def three_level_threshold(sse, w, h, B_max=16, B_min=4):
    """A finite threshold, read off the per-level SSE table {B: int [Rh, Rw]}, whose split holds at least one leaf of every
    side: just below the per-pixel error of one B_max block (so that block splits) for the first such block that leaves both a
    B_max leaf elsewhere and, inside it, leaves of both smaller sides.  Returns (threshold, leaves (x, y, B) in stream order)."""
    sides = set(qm.levels(B_max, B_min))
    for v in sorted({float(x) / (B_max * B_max) for x in sse[B_max].reshape(-1)}, reverse=True):
        t = float(np.nextafter(np.float32(v), np.float32(0.0)))
        tree = qm.split(sse, w, h, B_max, B_min, t)
        if {b for _, _, b in tree} == sides:
            return t, tree
    raise AssertionError("no threshold of the SSE table yields leaves of every side")
