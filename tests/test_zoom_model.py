"""Decoding at zoom, CPU side: the quadtree zoom models of tests/zoommodel.py against the existing
models at zoom 1 and against the oracle's own fixed-B decoders on a header-rescaled stream at zoom 2 and 4, and the checks the
zoom entries of the library make before they look for a device."""
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
from fic_amd import capi  # noqa: E402

INF = float("inf")


def _same(a, b):
    return bool(a[0].shape == b[0].shape and (a[0] == b[0]).all() and a[1].view(np.uint32) == b[1].view(np.uint32) and a[2] == b[2])


@pytest.fixture(scope="module")
def grey_streams(lena64, oracle):
    """{n_iso: (mixed-size stream, +inf stream, the fixed B = 16 rows and isometries)} of lena64, 16 -> 4, wK = 2."""
    h, w = lena64.shape
    out = {}
    for n_iso in (1, 8):
        cbs = qm.codebooks(lena64, 16, 4, 2, n_iso)
        sse = qm.level_sse(lena64, cbs, 2)
        t, tree = zm.three_level_threshold(sse, w, h)
        assert {b for _, _, b in tree} == {16, 8, 4}
        mixed = qm.write_run(qm.leaf_table(tree, cbs, w), w, h, 16, 4, 2, n_iso)
        inf = qm.write_run(qm.leaf_table(qm.split(sse, w, h, 16, 4, INF), cbs, w), w, h, 16, 4, 2, n_iso)
        out[n_iso] = (mixed, inf, cbs[16])
    return out


@pytest.fixture(scope="module")
def colour_streams(lena_colored, oracle):
    from oracle import fic_oracle as fo
    rgb = np.ascontiguousarray(lena_colored[64:128, 64:128])
    argb, w, h = fo.rgb_to_argb(rgb), 64, 64
    cbs = rm.codebooks(argb, w, h, 16, 4, 2)
    sse = rm.level_sse(argb, w, h, cbs, 2)
    t, tree = zm.three_level_threshold(sse, w, h)
    assert {b for _, _, b in tree} == {16, 8, 4}
    mixed = rm.write_run(rm.leaf_table(tree, cbs, w), w, h, 16, 4, 2)
    inf = rm.write_run(rm.leaf_table(rm.split(sse, w, h, 16, 4, INF), cbs, w), w, h, 16, 4, 2)
    return mixed, inf, cbs[16]


@pytest.mark.parametrize("n_iso", [1, 8])
def test_grey_zoom_model_at_1_is_the_quadtree_model(grey_streams, n_iso):
    for run in grey_streams[n_iso][:2]:
        assert _same(zm.decode_quadtree(run, 1), qm.decode(run))
    assert _same(zm.decode_quadtree(grey_streams[n_iso][0], 1, 3.25), qm.decode(grey_streams[n_iso][0], 3.25))


def test_colour_zoom_model_at_1_is_the_colour_model(colour_streams):
    for run in colour_streams[:2]:
        assert _same(zm.decode_rgb_quadtree(run, 1), rm.decode(run))


@pytest.mark.parametrize("z", [2, 4])
@pytest.mark.parametrize("n_iso", [1, 8])
def test_grey_inf_threshold_zoom_is_the_oracles_rescaled_fixed_decode(grey_streams, lena64, oracle, n_iso, z):
    """+inf: every leaf has side 16, and the zoom model must give what the reference arithmetic gives on the geometry
    (z*64, z*64, z*16, 2): pixels, avgError bits, iterations."""
    _, inf, (q16, k16) = grey_streams[n_iso]
    got = zm.decode_quadtree(inf, z)
    assert got[0].shape == (64 * z, 64 * z)
    assert _same(got, zm.decode_rows(q16, k16 if n_iso == 8 else None, 64, 64, 16, 2, z))
    if n_iso == 1:
        assert _same(got, zm.decode_gray(zm.fixed_run(0, q16, 64, 64, 16, 2), z))


@pytest.mark.parametrize("z", [2, 4])
def test_colour_inf_threshold_zoom_is_the_oracles_rescaled_fixed_decode(colour_streams, oracle, z):
    _, inf, q16 = colour_streams
    got = zm.decode_rgb_quadtree(inf, z)
    assert got[0].shape == (64 * z, 64 * z, 3)
    assert _same(got, zm.decode_rgb(zm.fixed_run(1, q16, 64, 64, 16, 2), z))


def test_mixed_streams_converge_at_every_zoom(grey_streams, colour_streams):
    for z in (1, 2, 4):
        for run, dec in ((grey_streams[1][0], zm.decode_quadtree), (grey_streams[8][0], zm.decode_quadtree),
                         (colour_streams[0], zm.decode_rgb_quadtree)):
            img, avg, it = dec(run, z)
            assert avg < 1 and it < 50 and img.shape[0] == 64 * z


# ---- the library's checks, all made before it looks for a device ------------------------------------------------------------
def _grey_run(w=64, h=64, B=8, wK=2):
    return zm.fixed_run(0, np.zeros(((w // B) * (h // B), 3), np.int32), w, h, B, wK)


def _colour_run(w=64, h=64, B=8, wK=2):
    return zm.fixed_run(1, np.zeros(((w // B) * (h // B), 5), np.int32), w, h, B, wK)


def _code(fn, *a, **k):
    with pytest.raises(fic_amd.FicError) as e:
        fn(*a, **k)
    return e.value.code


def test_library_declares_and_exports_the_zoom_entries():
    names = {"fic_decode_gray_run_zoom", "fic_decode_rgb_run_zoom", "fic_decode_quadtree_run_zoom",
             "fic_decode_rgb_quadtree_run_zoom", "fic_ctx_decode_zoom_host"}
    assert names <= set(capi.declared_symbols())
    for n in names:
        assert hasattr(capi.lib(), n)


@pytest.mark.parametrize("zoom", [0, 3, 8, -2])
def test_zoom_outside_1_2_4_is_an_argument_error(grey_streams, colour_streams, zoom):
    assert _code(fic_amd.decode_gray_run, _grey_run(), zoom=zoom) == -3
    assert _code(fic_amd.decode_rgb_run, _colour_run(), zoom=zoom) == -3
    assert _code(fic_amd.decode_quadtree_run, grey_streams[1][0], zoom=zoom) == -3
    assert _code(fic_amd.decode_rgb_quadtree_run, colour_streams[0], zoom=zoom) == -3


def test_zoomed_size_beyond_the_32_bit_limits_is_a_geometry_error():
    # 16384^2 is a valid geometry on its own (the header-only stream is refused for its length at zoom 1); 4x is 2^32 pixels
    hdr = struct.pack(">5i", 0, 16384, 16384, 16, 8)
    assert _code(fic_amd.decode_gray_run, hdr) == -3
    assert _code(fic_amd.decode_gray_run, hdr, zoom=2) == -3
    assert _code(fic_amd.decode_gray_run, hdr, zoom=4) == -1
    assert _code(fic_amd.decode_rgb_run, struct.pack(">5i", 1, 16384, 16384, 16, 8), zoom=4) == -1


def test_a_stream_must_be_encodable_itself_at_every_zoom():
    """The sides 32 and 64 exist for zoomed decodes only: a header that holds them is refused as before, whatever the zoom."""
    for z in (1, 2):
        assert _code(fic_amd.decode_gray_run, _grey_run(128, 128, 32), zoom=z) == -1
        assert _code(fic_amd.decode_rgb_run, _colour_run(128, 128, 32), zoom=z) == -1
    with pytest.raises(fic_amd.FicError):
        capi.geometry(128, 128, 32)


def test_short_output_is_a_capacity_error_with_the_zoomed_size_reported():
    import ctypes as C
    L = capi.lib()
    for run, fn, t in ((_grey_run(), L.fic_decode_gray_run_zoom, C.c_uint8), (_colour_run(), L.fic_decode_rgb_run_zoom, C.c_int32)):
        buf = np.frombuffer(run, np.uint8)
        out = np.zeros(128 * 128, np.uint8 if t is C.c_uint8 else np.int32)
        w, h = C.c_int(), C.c_int()
        rc = fn(capi.ptr(buf, C.c_uint8), buf.size, 2, 0, capi.ptr(out, t), 128 * 128 - 1, C.byref(w), C.byref(h), None, None)
        assert rc == -8 and (w.value, h.value) == (128, 128)
        rc = fn(capi.ptr(buf, C.c_uint8), buf.size, 1, 0, capi.ptr(out, t), 64 * 64 - 1, C.byref(w), C.byref(h), None, None)
        assert rc == -8 and (w.value, h.value) == (64, 64)


def test_quadtree_short_output_is_a_capacity_error(grey_streams, colour_streams):
    import ctypes as C
    L = capi.lib()
    for run, fn, t in ((grey_streams[1][0], L.fic_decode_quadtree_run_zoom, C.c_uint8),
                       (colour_streams[0], L.fic_decode_rgb_quadtree_run_zoom, C.c_int32)):
        buf = np.frombuffer(run, np.uint8)
        out = np.zeros(256 * 256, np.uint8 if t is C.c_uint8 else np.int32)
        w, h = C.c_int(), C.c_int()
        rc = fn(capi.ptr(buf, C.c_uint8), buf.size, 4, 0, capi.ptr(out, t), 256 * 256 - 1, C.byref(w), C.byref(h), None, None)
        assert rc == -8 and (w.value, h.value) == (256, 256)
