"""What every stream decoder of the C ABI refuses, and with which code: fic_decode_gray_run[_zoom], fic_debug_decode_gray_run,
fic_decode_rgb_run[_zoom], fic_decode_gray_iso_run, fic_decode_rgb_iso_run and the three quadtree readers, each on a hand-built
stream of its own tag (fixed block: 16 x 16, B = 4, wK = 2; quadtree: 32 x 32, levels 16..4, full search).  Codes only, never
message text.  After every refused call the caller's avgError and iteration count are untouched, and a correct decode through
the same entry right after it still matches the stream's model bit for bit -- pixels, avgError bits, iterations --, which a
workspace that did not come back intact would not."""
import ctypes as C
import os
import struct
import sys
from functools import lru_cache

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isostreammodel as im  # noqa: E402
import qtmodel as qm  # noqa: E402
import qtrgbmodel as rm  # noqa: E402
import streammodel as sm  # noqa: E402

from fic_amd import capi  # noqa: E402

pytestmark = pytest.mark.gpu

OK, GEOM, ARG, NOT_GREY, CAP = 0, -1, -3, -6, -8
CARRY = 3.25                     # avgError handed in: exact in float32, so "unchanged" is a comparison of bits
UNTOUCHED = -7                   # what the iteration count holds before every call
W, B, WK = 16, 4, 2              # the fixed-block streams
QW, B_MAX, B_MIN = 32, 16, 4     # the quadtree streams; wK = 0: the window of level B is its whole pool

# Leaves (x, y, B) in stream order: a leaf of side 16, four of side 8, a block split down to side 4, a leaf of side 16.
TREE = ([(0, 0, 16)] + [(16 + dx, dy, 8) for dx, dy in ((0, 0), (8, 0), (0, 8), (8, 8))]
        + [(0, 16, 8)] + [(8 + dx, 16 + dy, 4) for dx, dy in ((0, 0), (4, 0), (0, 4), (4, 4))] + [(0, 24, 8), (8, 24, 8)]
        + [(16, 16, 16)])


@lru_cache(maxsize=None)
def _quadtree_run(tag):
    """The tag-2 (n_iso = 8), tag-3 or tag-6 stream of TREE: rows as streammodel's cases draw them, leaf i with isometry i % 8."""
    rng = np.random.RandomState(40 + tag)
    n = len(TREE)
    leaves = np.zeros((n, {2: 7, 3: 8, 6: 9}[tag]), np.int32)
    leaves[:, :3] = np.array(TREE, np.int32)
    for i, (_, _, b) in enumerate(TREE):
        leaves[i, 3] = rng.randint(0, qm.level_wk(QW, QW, b, 0) ** 2)
    if tag == 2:
        leaves[:, 4] = rng.randint(-95, 96, n)
        leaves[:, 5] = rng.randint(-40, 301, n)
        leaves[:, 6] = np.arange(n) % 8
        return qm.write_run(leaves, QW, QW, B_MAX, B_MIN, 0, 8)
    leaves[:, 4] = rng.randint(-950000, 950001, n)
    leaves[:, 5] = rng.randint(-40, 301, n) * 100000 + rng.randint(0, 100000, n)
    leaves[:, 6] = rng.randint(-40, 301, n) * 100000 + rng.randint(0, 100000, n)
    leaves[:, 7] = rng.randint(-40, 301, n)
    if tag == 3:
        return rm.write_run(leaves, QW, QW, B_MAX, B_MIN, 0)
    leaves[:, 8] = np.arange(n) % 8
    return im.write_qt(leaves, QW, QW, B_MAX, B_MIN, 0)


@lru_cache(maxsize=None)
def _run(tag):
    if tag in (0, 1):
        return sm.fixed_case(tag, W, W, B, WK, 5 + tag)["run"]
    if tag in (4, 5):
        return im.fixed_case(tag, W, W, B, WK, 5 + tag)["run"]
    return _quadtree_run(tag)


def _reference(tag, z):
    return (sm if tag < 4 else im).reference(_run(tag), z, CARRY)


# The layout of a tag: header ints, ints per row, where the row's idx_local and isometry sit, the side of the image, a value
# of idx_local just outside the window (of the first row: the 1 x 1 pool of level 16 for the quadtrees), and the header int
# that must be 0.
class Layout:
    def __init__(self, hdr, per, idx_at, iso_at, side, idx_bad, zero_at):
        self.hdr, self.per, self.idx_at, self.iso_at, self.side, self.idx_bad, self.zero_at = hdr, per, idx_at, iso_at, side, idx_bad, zero_at


LAYOUT = {0: Layout(5, 3, 0, None, W, WK * WK, None), 1: Layout(5, 5, 0, None, W, WK * WK, None),
          4: Layout(6, 4, 0, 3, W, WK * WK, 3), 5: Layout(6, 6, 0, 5, W, WK * WK, 3),
          2: Layout(8, 5, 1, None, QW, 1, None), 3: Layout(8, 6, 1, None, QW, 1, 3), 6: Layout(8, 7, 1, 6, QW, 1, 3)}

# entry -> (tag it reads, takes a zoom, reports w_out / h_out, also reports seq_sums)
ENTRIES = {
    "fic_decode_gray_run": (0, False, True, False), "fic_decode_gray_run_zoom": (0, True, True, False),
    "fic_debug_decode_gray_run": (0, False, False, True),
    "fic_decode_rgb_run": (1, False, True, False), "fic_decode_rgb_run_zoom": (1, True, True, False),
    "fic_decode_gray_iso_run": (4, True, True, False), "fic_decode_rgb_iso_run": (5, True, True, False),
    "fic_decode_quadtree_run": (2, False, True, False), "fic_decode_quadtree_run_zoom": (2, True, True, False),
    "fic_decode_rgb_quadtree_run": (3, False, True, False), "fic_decode_rgb_quadtree_run_zoom": (3, True, True, False),
    "fic_decode_rgb_quadtree_iso_run": (6, True, True, False),
}
GREY = (0, 2, 4)


def _set(run, i, v):
    return run[:4 * i] + struct.pack(">i", v) + run[4 * i + 4:]


def _call(name, run, zoom=1, short=0):
    """One call of the entry with an output of zoom^2 side^2 - `short` pixels: (code, pixels, avgError, iterations, w_out, h_out);
    w_out / h_out stay None where the entry has none or did not write them."""
    tag, zoomed, sized, seq = ENTRIES[name]
    side = LAYOUT[tag].side * (zoom if zoom in (1, 2, 4) else 1)
    out = np.zeros(side * side, np.uint8 if tag in GREY else np.int32)
    buf = np.frombuffer(run, np.uint8) if len(run) else np.zeros(1, np.uint8)
    avg, it, w, h, sq = C.c_float(CARRY), C.c_int(UNTOUCHED), C.c_int(UNTOUCHED), C.c_int(UNTOUCHED), C.c_int(UNTOUCHED)
    args = [capi.ptr(buf, C.c_uint8), C.c_int64(len(run))] + ([C.c_int(zoom)] if zoomed else []) + \
           [C.c_int(0), capi.ptr(out, C.c_uint8 if tag in GREY else C.c_int32), C.c_int64(out.size - short)] + \
           ([C.byref(w), C.byref(h)] if sized else []) + [C.byref(avg), C.byref(it)] + ([C.byref(sq)] if seq else [])
    rc = getattr(capi.lib(), name)(*args)
    return rc, out.reshape(side, side), np.float32(avg.value), it.value, (w.value if w.value != UNTOUCHED else None), \
        (h.value if h.value != UNTOUCHED else None)


def _matches(tag, got, want):
    px = got[1] if tag in GREY else rm.channels(got[1], *got[1].shape[::-1])
    alpha = tag in GREY or (got[1].view(np.uint32) >> 24 == 0xFF).all()
    return bool(got[0] == OK and alpha and (px == want[0]).all()
                and np.float32(got[2]).view(np.uint32) == np.float32(want[1]).view(np.uint32) and got[3] == want[2])


def _cases(tag):
    """(name, stream, zoom, pixels the output is short of, code) of every refused call of a reader of `tag`; zoom None: the
    entry's own."""
    run, lay = _run(tag), LAYOUT[tag]
    other = {0: 1, 1: 0, 4: 5, 5: 4, 2: 3, 3: 6, 6: 3}[tag]
    out = [("shorter than the header", run[:4 * lay.hdr - 4], None, 0, ARG),
           ("empty", b"", None, 0, ARG),
           ("another tag", _run(other), None, 0, NOT_GREY if tag == 0 else ARG),
           ("its own body under another tag", _set(run, 0, other), None, 0, NOT_GREY if tag == 0 else ARG),
           ("a body one row short", run[:-4 * lay.per], None, 0, ARG),
           ("zoom 3", run, 3, 0, ARG),
           ("an output one pixel short", run, None, 1, CAP)]
    if lay.zero_at is not None:
        out.append(("a fourth header int that is not 0", _set(run, lay.zero_at, B if tag in (4, 5) else B_MAX), None, 0, ARG))
    if tag in (0, 1, 4, 5):      # a block side no encoder takes
        out.append(("a geometry the encoders refuse", _set(run, lay.hdr - 2, 5), None, 0, GEOM))
    else:                        # a width that is no multiple of B_max; the tag-3 reader reports every refused level as an argument
        out.append(("a geometry the encoders refuse", _set(run, 1, 40), None, 0, ARG if tag == 3 else GEOM))
    if tag not in (0, 1):
        out.append(("trailing bytes", run + bytes(4), None, 0, ARG))
    for bad in (-1, lay.idx_bad):
        # tags 0 and 1: found by the paint kernel's guard on the device, every other tag on the host
        out.append((f"idx_local {bad}", _set(run, lay.hdr + lay.idx_at, bad), None, 0, ARG))
    if lay.iso_at is not None:
        for bad in (-1, 8):
            out.append((f"isometry {bad}", _set(run, lay.hdr + lay.per * 2 + lay.iso_at, bad), None, 0, ARG))
    return out


@pytest.mark.parametrize("name", list(ENTRIES))
def test_refusals_and_the_decode_after_them(oracle, name):
    tag, zoomed, sized, _ = ENTRIES[name]
    run, lay = _run(tag), LAYOUT[tag]
    z0 = 2 if zoomed else 1
    want = _reference(tag, z0)
    assert _matches(tag, _call(name, run, z0), want), "the exact stream"
    for what, stream, zoom, short, code in _cases(tag):
        if zoom is not None and not zoomed:
            continue
        z = z0 if zoom is None else zoom
        rc, _, avg, it, w, h = _call(name, stream, z, short)
        assert rc == code, f"{what}: code {rc}"
        assert np.float32(avg).view(np.uint32) == np.float32(CARRY).view(np.uint32) and it == UNTOUCHED, f"{what}: avgError / iterations touched"
        if code == CAP and sized:
            assert (w, h) == (z * lay.side, z * lay.side), f"{what}: size reported as {w} x {h}"
        assert _matches(tag, _call(name, run, z0), want), f"the exact stream after {what}"
    if tag in (0, 1):            # the .run readers stop at the last row they need, as the reference's DataInputStream does
        got = _call(name, run + bytes(4), z0)
        assert _matches(tag, got, want) and (got[1] == _call(name, run, z0)[1]).all(), "trailing bytes"
        if sized:
            assert got[4:] == (z0 * lay.side, z0 * lay.side)
