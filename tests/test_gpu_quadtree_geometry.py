"""The quadtree encoders at the geometry edges, on the GPU against the numpy models on the CPU reference's own level codebooks:
grey (tag 2, n_iso 1 and 8, the image's red channel), colour (tag 3) and colour with isometries (tag 6, n_iso 1 and 8) on the
quadtree geometries of tests/geomcases.py -- a handful of top-level blocks, Rw != Rh both ways, windows of 1, 2, 3, 5 and the
whole pool -- with full-range noise and with S planes (blocks of SSE 0).

Unlike test_gpu_quadtree.py / test_gpu_rgb_quadtree.py the level codebooks come from the CPU (qtmodel.codebooks, the oracle's
encodeRGB per level, isostreammodel.codebooks), never from the GPU's one-shot entries: a level that is wrong in the same way in
the one-shot path and in the quadtree path shows here, in the per-level SSE hook first.

Leaves are compared at +inf, -1, +0.0, -0.0, a threshold with leaves of every side, and for every level above B_min at the
boundary pair t = float32(s / B^2) and its float32 predecessor, s the SSE of the level's boundary block (geomcases.qt_boundary):
`(double) s > (double) t * B * B` is an equality there, so the block is a leaf at t and split just below; `>=`, or a product
rounded to float, moves it.  Streams equal the models' writers byte for byte; decodes (pixels, avgError bits, iterations) equal
the models' at +inf, -1 and the three-level threshold, the latter also at zoom 2; at +inf the rows are the level codebook in
scanline order and the stream decodes like the fixed-B_max stream of tag 0 / 4 / 1 / 5."""
import numpy as np
import pytest

import geomcases as gc
import isostreammodel as im
import qtmodel as qm
import qtrgbmodel as qr
import zoommodel as zm
from fic_amd import capi

pytestmark = pytest.mark.gpu
INF = float("inf")


class _Grey:
    """tag 2"""
    def __init__(self, c, ref):
        self.c, self.ref, self.n_iso, self.g = c, ref, ref["n_iso"], ref["gray"]

    def sse(self):
        return capi.debug_quadtree_sse(self.g, self.c.B_max, self.c.B_min, self.c.wK, self.n_iso)

    def encode(self, t):
        return capi.encode_gray_quadtree(self.g, self.c.B_max, self.c.B_min, self.c.wK, self.n_iso, t)

    def write(self, leaves):
        c = self.c
        return capi.write_run_quadtree(leaves, c.w, c.h, c.B_max, c.B_min, c.wK, self.n_iso), \
            qm.write_run(leaves, c.w, c.h, c.B_max, c.B_min, c.wK, self.n_iso)

    def decode(self, run, z):
        return capi.decode_quadtree_run(run, zoom=z), zm.decode_quadtree(run, z)

    def fixed(self):
        c, (q, k) = self.c, self.ref["cbs"][self.c.B_max]
        wk = qm.level_wk(c.w, c.h, c.B_max, c.wK)
        if self.n_iso == 1:
            return q, capi.decode_gray_run(capi.write_run_gray(q, c.w, c.h, c.B_max, wk))
        return np.concatenate([q, k[:, None]], axis=1), capi.decode_gray_iso_run(capi.write_run_gray_iso(q, k, c.w, c.h, c.B_max, wk))


class _Rgb:
    """tag 3"""
    def __init__(self, c, ref):
        self.c, self.ref, self.n_iso, self.a = c, ref, 1, ref["argb"]

    def sse(self):
        return capi.debug_rgb_quadtree_sse(self.a, self.c.w, self.c.h, self.c.B_max, self.c.B_min, self.c.wK)

    def encode(self, t):
        return capi.encode_rgb_quadtree(self.a, self.c.w, self.c.h, self.c.B_max, self.c.B_min, self.c.wK, t)

    def write(self, leaves):
        c = self.c
        return capi.write_run_rgb_quadtree(leaves, c.w, c.h, c.B_max, c.B_min, c.wK), qr.write_run(leaves, c.w, c.h, c.B_max, c.B_min, c.wK)

    def decode(self, run, z):
        return capi.decode_rgb_quadtree_run(run, zoom=z), zm.decode_rgb_quadtree(run, z)

    def fixed(self):
        c, q = self.c, self.ref["cbs"][self.c.B_max]
        out, avg, it, w, h = capi.decode_rgb_run(capi.write_run_rgb(q, c.w, c.h, c.B_max, qm.level_wk(c.w, c.h, c.B_max, c.wK)))
        return q, (out.reshape(h, w), avg, it)


class _RgbIso(_Rgb):
    """tag 6"""
    def __init__(self, c, ref):
        self.c, self.ref, self.n_iso, self.a = c, ref, ref["n_iso"], ref["argb"]

    def sse(self):
        return capi.debug_rgb_quadtree_iso_sse(self.a, self.c.w, self.c.h, self.c.B_max, self.c.B_min, self.c.wK, self.n_iso)

    def encode(self, t):
        return capi.encode_rgb_quadtree_iso(self.a, self.c.w, self.c.h, self.c.B_max, self.c.B_min, self.c.wK, self.n_iso, t)

    def write(self, leaves):
        c = self.c
        return capi.write_run_rgb_quadtree_iso(leaves, c.w, c.h, c.B_max, c.B_min, c.wK), im.write_qt(leaves, c.w, c.h, c.B_max, c.B_min, c.wK)

    def decode(self, run, z):
        return capi.decode_rgb_quadtree_iso_run(run, zoom=z), im.decode_qt(run, z)

    def fixed(self):
        c, (q, k) = self.c, self.ref["cbs"][self.c.B_max]
        run = capi.write_run_rgb_iso(q, k, c.w, c.h, c.B_max, qm.level_wk(c.w, c.h, c.B_max, c.wK))
        out, avg, it, w, h = capi.decode_rgb_iso_run(run)
        return np.concatenate([q, k[:, None]], axis=1), (out.reshape(h, w), avg, it)


def _same_decode(got, want):
    """GPU (gray uint8 [h, w] or argb int32 [h, w], avg, it) against the model's (gray or rgb [h, w, 3], avg, it)."""
    px = got[0]
    if px.dtype != np.uint8:
        h, w = px.shape
        if not (px.view(np.uint32) >> 24 == 0xFF).all():
            return False
        px = qr.channels(px, w, h)
    return bool((px == want[0]).all() and np.float32(got[1]).view(np.uint32) == np.float32(want[1]).view(np.uint32) and got[2] == want[2])


@pytest.mark.parametrize("encoder", gc.QT_ENCODERS)
@pytest.mark.parametrize("c", gc.QT_CASES, ids=gc.qt_case_id)
def test_quadtree_geometry(c, encoder):
    cid = f"{gc.qt_case_id(c)} {encoder}"
    ref = gc.qt_reference(c, encoder)
    E = (_Grey if encoder.startswith("grey") else _Rgb if encoder == "rgb" else _RgbIso)(c, ref)
    sse, levels = ref["sse"], qm.levels(c.B_max, c.B_min)
    got = E.sse()
    for B in levels:
        bad = np.flatnonzero(got[B].astype(np.int64).reshape(-1) != sse[B].reshape(-1))
        assert bad.size == 0, f"{cid}: SSE at B={B} differs first at block {bad[0]}: {got[B].reshape(-1)[bad[0]]}, model {sse[B].reshape(-1)[bad[0]]}"

    def leaves_at(t, what):
        tree = qm.split(sse, c.w, c.h, c.B_max, c.B_min, t)
        want = gc.qt_leaf_table(c, encoder, tree)
        leaves = E.encode(t)
        assert leaves.shape == want.shape, f"{cid}: {len(leaves)} leaves at {what} = {t!r}, model {len(want)}"
        bad = np.flatnonzero((leaves != want).any(axis=1))
        assert bad.size == 0, f"{cid}: leaf {bad[0]} at {what} = {t!r}: {leaves[bad[0]]}, model {want[bad[0]]}"
        return leaves, tree

    def streams_and_decode(leaves, what, zooms=(1,)):
        run, want = E.write(leaves)
        assert run == want, f"{cid}: stream bytes at {what}"
        dec = None
        for z in zooms:
            g, m = E.decode(run, z)
            assert _same_decode(g, m), f"{cid}: decode at {what}, zoom {z}"
            dec = dec or g
        return dec

    # +inf: the level codebook of B_max in scanline order; the stream decodes like the fixed-B_max stream
    leaves, tree = leaves_at(INF, "+inf")
    rows, fixed = E.fixed()
    assert (leaves[:, 2] == c.B_max).all() and (leaves[:, 3:3 + rows.shape[1]] == rows).all(), f"{cid}: rows at +inf"
    dec = streams_and_decode(leaves, "+inf")
    assert (dec[0] == fixed[0]).all() and np.float32(dec[1]).view(np.uint32) == np.float32(fixed[1]).view(np.uint32) and dec[2] == fixed[2], \
        f"{cid}: the +inf stream against the fixed-B_max stream"
    # -1: every B_min block
    leaves, tree = leaves_at(-1.0, "-1")
    assert (leaves[:, 2] == c.B_min).all() and len(leaves) == (c.w // c.B_min) * (c.h // c.B_min)
    streams_and_decode(leaves, "-1")
    # both zeros: a block of SSE 0 is never split
    plus, tree = leaves_at(0.0, "+0.0")
    minus, _ = leaves_at(-0.0, "-0.0")
    assert (plus == minus).all()
    if c.kind == "S":
        whole = {(x, y, B) for x, y, B in tree if B > c.B_min}
        assert whole and all(sse[B][y // B, x // B] == 0 for x, y, B in whole), f"{cid}: leaves above B_min at threshold 0"
    # leaves of every side, decoded at zoom 1 and 2
    t3, tree = zm.three_level_threshold(sse, c.w, c.h, c.B_max, c.B_min)
    leaves, _ = leaves_at(t3, "the three-level threshold")
    assert set(leaves[:, 2]) == set(levels), f"{cid}: sides {set(leaves[:, 2])}"
    streams_and_decode(leaves, "the three-level threshold", zooms=(1, 2))
    # the split rule at equality, level by level
    for B in levels[:-1]:
        x, y, s, t = gc.qt_boundary(c, sse, B)
        at, _ = leaves_at(t, f"the boundary of B={B} (s={s})")
        below, _ = leaves_at(np.nextafter(t, np.float32(-np.inf)), f"just below the boundary of B={B} (s={s})")
        is_leaf = lambda lv: bool(((lv[:, 0] == x) & (lv[:, 1] == y) & (lv[:, 2] == B)).any())  # noqa: E731
        assert is_leaf(at) and not is_leaf(below) and len(below) > len(at), f"{cid}: boundary block ({x}, {y}) of B={B}"
