"""Decoding at zoom 1, 2 and 4 on the GPU against the reference models of tests/zoommodel.py: the
oracle's own decoders on a header-rescaled stream for the fixed-B entries, the numpy quadtree loops with leaves and geometry
multiplied by the zoom for the quadtree entries.  Every comparison is exact: pixels, avgError as a bit pattern, iterations.
The effective block sides are 4 .. 64; 32 and 64 are painted in row segments (k_decode_paint<32 / 64>,
k_decode_paint_leaves<Fmt, 32 / 64>)."""
import ctypes as C
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qtmodel as qm  # noqa: E402
import qtrgbmodel as rm  # noqa: E402
import zoommodel as zm  # noqa: E402

import fic_amd  # noqa: E402
from fic_amd import capi, synth  # noqa: E402
from oracle import fic_oracle as fo  # noqa: E402

pytestmark = pytest.mark.gpu

INF = float("inf")
ZOOMS = (1, 2, 4)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _same(got, want):
    """(pixels, avgError, iterations) of a grey decode, or of a colour model decode, bit for bit."""
    return bool(got[0].shape == want[0].shape and (got[0] == want[0]).all()
                and np.float32(got[1]).view(np.uint32) == np.float32(want[1]).view(np.uint32) and got[2] == want[2])


def _same_rgb(argb, avg, it, want):
    """A GPU colour decode (packed ARGB of any shape) against a model's (rgb [h, w, 3], avgError, iterations)."""
    h, w = want[0].shape[:2]
    return bool(argb.size == w * h and (rm.channels(argb, w, h) == want[0]).all() and (argb.view(np.uint32) >> 24 == 0xFF).all()
                and np.float32(avg).view(np.uint32) == np.float32(want[1]).view(np.uint32) and it == want[2])


def _grey_run(gray, B, wK):
    """The .run stream of the GPU's own encode of `gray` (wK None: full search)."""
    h, w = gray.shape
    wk = capi.geometry(w, h, B)[2] if wK is None else wK
    return fic_amd.write_run_gray(capi.encode_gray_oneshot(gray, B, wk)["qrows"], w, h, B, wk)


# ---- fixed-B grey runs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wK", [None, 8])
@pytest.mark.parametrize("name,B", [("lena64", 4), ("lena64", 8), ("lena_grey_256", 8), ("lena_grey_256", 16)])
def test_grey_runs_at_every_zoom(oracle, lena64, lena_grey, name, B, wK):
    run = _grey_run(lena64 if name == "lena64" else lena_grey, B, wK)
    for z in ZOOMS:
        got, want = fic_amd.decode_gray_run(run, zoom=z), zm.decode_gray(run, z)
        print(f"{name} B={B} wK={wK} zoom={z}: B'={z * B} iterations {got[2]} / {want[2]} avgError {got[1]!r} / {want[1]!r}")
        assert _same(got, want), (name, B, wK, z)
        assert want[1] < 1


# ---- the reference's own colour stream -------------------------------------------------------------------------------------------
def test_colour_run_of_the_reference_at_every_zoom(oracle):
    run = open(os.path.join(GOLDEN, "unknown_run.bin"), "rb").read()
    for z in ZOOMS:
        argb, avg, it, w, h = fic_amd.decode_rgb_run(run, zoom=z)
        want = zm.decode_rgb(run, z)
        print(f"unknown_run zoom={z}: {w}x{h} iterations {it} / {want[2]} avgError {avg!r} / {want[1]!r}")
        assert (w, h) == (256 * z, 256 * z) and _same_rgb(argb, avg, it, want), z


# ---- non-square images: scaleImage's `x + 1 >= height` at the zoomed size -------------------------------------------------------
@pytest.mark.parametrize("w,h", [(128, 64), (64, 128)])
def test_non_square_images_at_every_zoom(oracle, w, h):
    gray = synth.image("S", w, h, synth.SEEDS["cfg5"] + w + 7 * h)
    assert gray.shape == (h, w)
    run = _grey_run(gray, 8, 4)
    rgb = np.stack([synth.image("S" if c else "U", w, h, synth.SEEDS["cfg5"] + 3 * w + h + c) for c in range(3)], axis=-1)
    crun = fic_amd.write_run_rgb(capi.encode_rgb(fo.rgb_to_argb(rgb), w, h, 8, 2)["qrows"], w, h, 8, 2)
    for z in ZOOMS:
        assert _same(fic_amd.decode_gray_run(run, zoom=z), zm.decode_gray(run, z)), ("grey", w, h, z)
        argb, avg, it, zw, zh = fic_amd.decode_rgb_run(crun, zoom=z)
        assert (zw, zh) == (z * w, z * h) and _same_rgb(argb, avg, it, zm.decode_rgb(crun, z)), ("colour", w, h, z)


# ---- the context's own codebook: isometries and batched planes ----------------------------------------------------------------
@pytest.mark.parametrize("B,wK", [(8, None), (16, 3), (4, 5)])
def test_context_decode_with_isometries_and_planes(oracle, lena_grey, B, wK):
    planes = np.stack([lena_grey[:128, :128], synth.image("S", 128, 128, 11), lena_grey[128:, 64:192]])
    with fic_amd.Encoder(128, 128, B, wK, 8, planes=3) as enc:
        enc.set_gray(planes)
        enc.encode()
        r = enc.results()
        wk = capi.geometry(128, 128, B)[2] if wK is None else wK
        assert len(set(r["iso"].reshape(-1))) > 1
        plain = enc.decode()
        for z in ZOOMS:
            img, avg, it = enc.decode(zoom=z)
            assert img.shape == (3, 128 * z, 128 * z)
            for p in range(3):
                want = zm.decode_rows(r["qrows"][p], r["iso"][p], 128, 128, B, wk, z)
                assert _same((img[p], avg[p], it[p]), want), (B, wK, z, p)
            if z == 1:
                assert (img == plain[0]).all() and (avg.view(np.uint32) == plain[1].view(np.uint32)).all() and (it == plain[2]).all()
        with pytest.raises(fic_amd.FicError) as e:
            enc.decode(zoom=3)
        assert e.value.code == -3


# ---- quadtree streams ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_iso", [1, 8])
def test_grey_quadtree_streams_at_every_zoom(oracle, lena64, n_iso):
    h, w = lena64.shape
    cbs = {}
    for B in (16, 8, 4):
        wk = qm.level_wk(w, h, B, 0)
        with fic_amd.Encoder(w, h, B, wk, n_iso) as enc:
            enc.set_gray(lena64)
            enc.encode()
            r = enc.results()
        cbs[B] = (r["qrows"][0], r["iso"][0])
    sse = qm.level_sse(lena64, cbs, 0)
    t, tree = zm.three_level_threshold(sse, w, h)
    assert np.isfinite(t) and {b for _, _, b in tree} == {16, 8, 4}
    for thr in (t, INF):
        leaves = fic_amd.encode_gray_quadtree(lena64, 16, 4, 0, n_iso, thr)
        assert (leaves == qm.leaf_table(qm.split(sse, w, h, 16, 4, thr), cbs, w)).all()
        assert {int(b) for b in leaves[:, 2]} == ({16, 8, 4} if thr == t else {16})
        run = fic_amd.write_run_quadtree(leaves, w, h, 16, 4, 0, n_iso)
        for z in ZOOMS:
            assert _same(fic_amd.decode_quadtree_run(run, zoom=z), zm.decode_quadtree(run, z)), (n_iso, thr, z)
        assert _same(fic_amd.decode_quadtree_run(run, zoom=1), fic_amd.decode_quadtree_run(run))
        assert _same(fic_amd.decode_quadtree_run(run, avg_error_in=2.5, zoom=4), zm.decode_quadtree(run, 4, 2.5))


def test_colour_quadtree_streams_at_every_zoom(oracle, lena_colored):
    rgb = np.ascontiguousarray(lena_colored[64:192, 64:192])
    argb, w, h = fo.rgb_to_argb(rgb), 128, 128
    cbs = {B: capi.encode_rgb(argb, w, h, B, rm.level_wk(w, h, B, 0))["qrows"] for B in (16, 8, 4)}
    sse = rm.level_sse(argb, w, h, cbs, 0)
    t, tree = zm.three_level_threshold(sse, w, h)
    assert np.isfinite(t) and {b for _, _, b in tree} == {16, 8, 4}
    for thr in (t, INF):
        leaves = fic_amd.encode_rgb_quadtree(argb, w, h, 16, 4, 0, thr)
        assert (leaves == rm.leaf_table(rm.split(sse, w, h, 16, 4, thr), cbs, w)).all()
        assert {int(b) for b in leaves[:, 2]} == ({16, 8, 4} if thr == t else {16})
        run = fic_amd.write_run_rgb_quadtree(leaves, w, h, 16, 4, 0)
        for z in ZOOMS:
            img, avg, it = fic_amd.decode_rgb_quadtree_run(run, zoom=z)
            assert img.shape == (z * h, z * w) and _same_rgb(img, avg, it, zm.decode_rgb_quadtree(run, z)), (thr, z)
        a, b = fic_amd.decode_rgb_quadtree_run(run, zoom=1), fic_amd.decode_rgb_quadtree_run(run)
        assert (a[0] == b[0]).all() and a[1].view(np.uint32) == b[1].view(np.uint32) and a[2] == b[2]
        img, avg, it = fic_amd.decode_rgb_quadtree_run(run, avg_error_in=2.5, zoom=2)
        assert _same_rgb(img, avg, it, zm.decode_rgb_quadtree(run, 2, 2.5))


# ---- a carried-in avgError (FC:20: the static is never reset) --------------------------------------------------------------------
@pytest.mark.parametrize("carry", [3.25, 1.0e7, 0.75])
def test_non_zero_avg_error_in(oracle, lena64, carry):
    run = _grey_run(lena64, 8, 8)
    crun = open(os.path.join(GOLDEN, "unknown_run.bin"), "rb").read()
    for z in (2, 4):
        assert _same(fic_amd.decode_gray_run(run, avg_error_in=carry, zoom=z), zm.decode_gray(run, z, carry)), z
    argb, avg, it, w, h = fic_amd.decode_rgb_run(crun, avg_error_in=carry, zoom=2)
    assert _same_rgb(argb, avg, it, zm.decode_rgb(crun, 2, carry))


# ---- consistency with the unzoomed entries ---------------------------------------------------------------------------------------
def test_zoom_1_is_the_unzoomed_entry_and_zoom_2_is_the_rescaled_header(oracle, lena64, lena_grey):
    for gray, B in ((lena64, 4), (lena64, 8), (lena_grey, 16)):
        run = _grey_run(gray, B, 8)
        assert _same(fic_amd.decode_gray_run(run, zoom=1), fic_amd.decode_gray_run(run))
        assert _same(fic_amd.decode_gray_run(run, avg_error_in=5.5, zoom=1), fic_amd.decode_gray_run(run, avg_error_in=5.5))
    run = _grey_run(lena_grey, 8, 8)
    assert _same(fic_amd.decode_gray_run(run, zoom=2), fic_amd.decode_gray_run(zm.rescale_header(run, 2)))
    run = _grey_run(lena64, 4, 8)
    assert _same(fic_amd.decode_gray_run(run, zoom=4), fic_amd.decode_gray_run(zm.rescale_header(run, 4)))
    assert _same(fic_amd.decode_gray_run(run, zoom=2), fic_amd.decode_gray_run(zm.rescale_header(run, 2)))
    crun = open(os.path.join(GOLDEN, "unknown_run.bin"), "rb").read()
    a, b = fic_amd.decode_rgb_run(crun, zoom=1), fic_amd.decode_rgb_run(crun)
    assert (a[0] == b[0]).all() and a[1].view(np.uint32) == b[1].view(np.uint32) and a[2:] == b[2:]
    a, b = fic_amd.decode_rgb_run(crun, zoom=2), fic_amd.decode_rgb_run(zm.rescale_header(crun, 2))     # B = 8 -> 16
    assert (a[0] == b[0]).all() and a[1].view(np.uint32) == b[1].view(np.uint32) and a[2:] == b[2:]


# ---- error paths -----------------------------------------------------------------------------------------------------------------
def _code(fn, *a, **k):
    with pytest.raises(fic_amd.FicError) as e:
        fn(*a, **k)
    return e.value.code


def test_error_codes(oracle, lena64):
    run = _grey_run(lena64, 8, 8)
    crun = open(os.path.join(GOLDEN, "unknown_run.bin"), "rb").read()
    leaves = fic_amd.encode_gray_quadtree(lena64, 16, 4, 0, 1, 100.0)
    qrun = fic_amd.write_run_quadtree(leaves, 64, 64, 16, 4, 0, 1)
    argb = fo.rgb_to_argb(np.stack([lena64] * 3, axis=-1))
    cqrun = fic_amd.write_run_rgb_quadtree(fic_amd.encode_rgb_quadtree(argb, 64, 64, 16, 4, 0, 100.0), 64, 64, 16, 4, 0)
    entries = ((fic_amd.decode_gray_run, run), (fic_amd.decode_rgb_run, crun), (fic_amd.decode_quadtree_run, qrun),
               (fic_amd.decode_rgb_quadtree_run, cqrun))
    for fn, s in entries:                                                 # FIC_E_ARGUMENT: a zoom outside {1, 2, 4}
        for z in (0, 3, 8, -1):
            assert _code(fn, s, zoom=z) == -3, (fn.__name__, z)
    big = struct.pack(">5i", 0, 16384, 16384, 16, 8)                      # FIC_E_GEOMETRY: 65536^2 pixels at zoom 4
    assert _code(fic_amd.decode_gray_run, big, zoom=4) == -1
    assert _code(fic_amd.decode_rgb_run, struct.pack(">5i", 1, 16384, 16384, 16, 8), zoom=4) == -1
    assert _code(fic_amd.decode_gray_run, zm.rescale_header(run, 4), zoom=2) == -1    # the stream's own B = 32
    L = capi.lib()                                                        # FIC_E_CAPACITY: one pixel short of zoom^2 * w * h
    for fn, s, t, n in ((L.fic_decode_gray_run_zoom, run, np.uint8, 64), (L.fic_decode_rgb_run_zoom, crun, np.int32, 256),
                        (L.fic_decode_quadtree_run_zoom, qrun, np.uint8, 64), (L.fic_decode_rgb_quadtree_run_zoom, cqrun, np.int32, 64)):
        buf = np.frombuffer(s, np.uint8)
        out = np.zeros(4 * n * n, t)
        w, h = C.c_int(), C.c_int()
        p = capi.ptr(out, C.c_uint8 if t is np.uint8 else C.c_int32)
        assert fn(capi.ptr(buf, C.c_uint8), buf.size, 2, 0, p, 4 * n * n - 1, C.byref(w), C.byref(h), None, None) == -8
        assert (w.value, h.value) == (2 * n, 2 * n)
        assert fn(capi.ptr(buf, C.c_uint8), buf.size, 2, 0, p, 4 * n * n, C.byref(w), C.byref(h), None, None) == 0
    # FIC_E_ARGUMENT: a row that points outside the pool, exactly as at zoom 1 (wK = 8 window of a 13 x 13 pool: index 64)
    bad = bytearray(run)
    bad[20 + 12 * 5:24 + 12 * 5] = (64).to_bytes(4, "big")
    for z in ZOOMS:
        assert _code(fic_amd.decode_gray_run, bytes(bad), zoom=z) == -3, z
    assert _code(fic_amd.decode_gray_run, bytes(bad)) == -3
    cbad = bytearray(crun)
    cbad[20 + 20 * 7:24 + 20 * 7] = (10 ** 6).to_bytes(4, "big")
    for z in ZOOMS:
        assert _code(fic_amd.decode_rgb_run, bytes(cbad), zoom=z) == -3, z


# ---- one large case: 4096 x 4096 with block side 64 ------------------------------------------------------------------------------
def test_large_grey_1024_at_zoom_4(oracle, lena_grey):
    gray = np.ascontiguousarray(np.tile(lena_grey, (4, 4)))
    assert gray.shape == (1024, 1024)
    run = _grey_run(gray, 16, None)
    got = fic_amd.decode_gray_run(run, zoom=4)
    want = zm.decode_gray(run, 4)
    print(f"1024^2 B=16 zoom=4: iterations {got[2]} / {want[2]} avgError {got[1]!r} / {want[1]!r}")
    assert got[0].shape == (4096, 4096) and _same(got, want)
