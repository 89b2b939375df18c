"""Streams with an isometry column, CPU side: the library's host-only writers against
tests/isostreammodel.py, every refusal the readers make before they look for a device, the refusals of the four older readers,
and the model's own identities -- a column of zeros decodes like the tag-0 / 1 / 3 twin at every zoom, n_iso = 1 gives the
colour quadtree's leaves, and on the hand-built tag-6 cases every (side, isometry) pair shows in the decoded pixels, so the GPU
tests of tests/test_gpu_iso_streams.py cannot pass with a painter that ignores, swaps or mis-sizes an isometry.  No GPU."""
import ctypes as C
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isostreammodel as im  # noqa: E402
import qtmodel as qm  # noqa: E402
import qtrgbmodel as rm  # noqa: E402
import streammodel as sm  # noqa: E402
import zoommodel as zm  # noqa: E402

import fic_amd  # noqa: E402
from fic_amd import capi  # noqa: E402

ARG, GEOM, WIN, NOT_GREY, CAP = -3, -1, -2, -6, -8
ZOOMS = (1, 2, 4)
NEW = {"fic_write_run_gray_iso", "fic_write_run_rgb_iso", "fic_write_run_rgb_quadtree_iso", "fic_decode_gray_iso_run",
       "fic_decode_rgb_iso_run", "fic_decode_rgb_quadtree_iso_run", "fic_rgb_ctx_decode_zoom_host",
       "fic_encode_rgb_quadtree_iso_argb", "fic_debug_rgb_quadtree_iso_sse"}


def _same(a, b):
    return bool(a[0].shape == b[0].shape and (a[0] == b[0]).all() and np.float32(a[1]).view(np.uint32) == np.float32(b[1]).view(np.uint32)
                and a[2] == b[2])


def _code(fn, *a, **k):
    with pytest.raises(fic_amd.FicError) as e:
        fn(*a, **k)
    return e.value.code


def _leaf(img, leaf, z):
    x, y, B = (int(v) * z for v in leaf[:3])
    return img[y:y + B, x:x + B]


def test_library_declares_and_exports_the_new_entries():
    assert NEW <= set(capi.declared_symbols())
    for n in NEW:
        assert hasattr(capi.lib(), n)


# ---- writers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,w,h,B,wK", [(4, 64, 64, 4, 0), (4, 128, 64, 16, 2), (5, 64, 64, 8, 0), (5, 128, 64, 4, 2)])
def test_fixed_writer_bytes_and_round_trip(oracle, tag, w, h, B, wK):
    c = im.fixed_case(tag, w, h, B, wK, 3)
    write = fic_amd.write_run_gray_iso if tag == 4 else fic_amd.write_run_rgb_iso
    run = write(c["rows"], c["iso"], w, h, B, c["wK"])
    assert run == c["run"] and len(run) == 24 + 4 * (im.FIXED_QW[tag] + 1) * len(c["rows"])
    hd, rows, iso = im.read_fixed(run)
    assert hd == dict(tag=tag, w=w, h=h, B=B, wK=c["wK"]) and (rows == c["rows"]).all() and (iso == c["iso"]).all()
    assert set(iso.tolist()) == set(range(8))
    assert write(c["rows"], np.zeros_like(c["iso"]), w, h, B, c["wK"]) == im.write_fixed(tag, c["rows"], np.zeros_like(c["iso"]), w, h, B, c["wK"])


@pytest.mark.parametrize("w,h,wK,seed", im.QT_CASES)
def test_quadtree_writer_bytes_and_round_trip(oracle, w, h, wK, seed):
    c = im.quadtree_case(w, h, wK, seed)
    run = fic_amd.write_run_rgb_quadtree_iso(c["leaves"], w, h, 16, 4, wK)
    assert run == c["run"] and len(run) == 32 + 28 * len(c["leaves"])
    hd, leaves = im.read_qt(run)
    assert hd == dict(w=w, h=h, B_max=16, B_min=4, wK=wK) and (leaves == c["leaves"]).all()
    assert {(int(b), int(k)) for b, k in leaves[:, [2, 8]]} == {(b, k) for b in (4, 8, 16) for k in range(8)}
    # the tree, the rows and the designated leaves are those of the tag-3 case
    assert im.tag3_twin(run) == sm.rgb_quadtree_case(w, h, wK, seed)["run"]


def test_fixed_writers_refuse(oracle):
    L = capi.lib()
    for tag, fn in ((4, L.fic_write_run_gray_iso), (5, L.fic_write_run_rgb_iso)):
        c = im.fixed_case(tag, 64, 64, 8, 2, 3)
        q, k = np.ascontiguousarray(c["rows"], np.int32), np.ascontiguousarray(c["iso"], np.int32)
        n = len(q)
        out = np.zeros(len(c["run"]), np.uint8)
        P = lambda a, t=C.c_int32: capi.ptr(a, t)  # noqa: E731

        def call(qq=q, kk=k, nn=n, w=64, h=64, B=8, wK=2, o=out, cap=None):
            return int(fn(P(qq), P(kk), nn, w, h, B, wK, P(o, C.c_uint8), o.size if cap is None else cap))

        assert call() == len(c["run"]) and out.tobytes() == c["run"]
        assert int(fn(None, P(k), n, 64, 64, 8, 2, P(out, C.c_uint8), out.size)) == ARG
        assert int(fn(P(q), None, n, 64, 64, 8, 2, P(out, C.c_uint8), out.size)) == ARG
        assert int(fn(P(q), P(k), n, 64, 64, 8, 2, None, out.size)) == ARG
        for bad in (-1, 8):
            kb = k.copy()
            kb[n // 2] = bad
            assert call(kk=kb) == ARG
        assert call(nn=n - 1) == ARG and call(nn=n + 1) == ARG and call(nn=0) == ARG
        assert call(B=5) == GEOM and call(w=60) == GEOM and call(w=0) == GEOM
        assert call(wK=0) == WIN and call(wK=14) == WIN
        assert call(cap=len(c["run"]) - 1) == CAP


def test_quadtree_writer_refuses(oracle):
    c = im.quadtree_case(*im.QT_CASES[1])
    w, h, wK, lv = c["w"], c["h"], c["wK"], c["leaves"]
    W = fic_amd.write_run_rgb_quadtree_iso
    for bad in (-1, 8):
        b = lv.copy()
        b[5, 8] = bad
        assert _code(W, b, w, h, 16, 4, wK) == ARG
    assert _code(W, lv[:-1], w, h, 16, 4, wK) == ARG                        # does not tile
    sw = lv.copy()
    sw[[0, 1]] = sw[[1, 0]]
    assert _code(W, sw, w, h, 16, 4, wK) == ARG                             # not in quadtree order
    assert _code(W, lv, w, h, 16, 16, wK) == ARG and _code(W, lv, w, h, 32, 4, wK) == ARG
    assert _code(W, lv, w + 8, h, 16, 4, wK) == GEOM
    assert _code(W, lv, w, h, 16, 4, -1) == WIN and _code(W, lv, w, h, 16, 4, 0) == WIN      # full search needs a square image
    L = capi.lib()
    q = np.ascontiguousarray(lv, np.int32)
    out = np.zeros(len(c["run"]), np.uint8)
    assert int(L.fic_write_run_rgb_quadtree_iso(capi.ptr(q, C.c_int32), len(q), w, h, 16, 4, wK, capi.ptr(out, C.c_uint8), out.size - 1)) == CAP
    assert int(L.fic_write_run_rgb_quadtree_iso(None, len(q), w, h, 16, 4, wK, capi.ptr(out, C.c_uint8), out.size)) == ARG


# ---- readers: everything is refused on the host, before any device work ------------------------------------------------------
def _set(run, i, v):
    return run[:4 * i] + struct.pack(">i", v) + run[4 * i + 4:]


@pytest.mark.parametrize("tag", [4, 5])
def test_fixed_readers_refuse_malformed_streams(oracle, tag):
    c = im.fixed_case(tag, 128, 64, 8, 2, 3)
    run, per = c["run"], im.FIXED_QW[tag] + 1
    dec = fic_amd.decode_gray_iso_run if tag == 4 else fic_amd.decode_rgb_iso_run
    for other in (0, 1, 2, 3, 6, 9 - tag, -1):
        assert _code(dec, _set(run, 0, other)) == ARG
    assert _code(dec, _set(run, 3, 8)) == ARG                                # a .run's block size where the 0 belongs
    assert _code(dec, run[:-4]) == ARG and _code(dec, run + bytes(4)) == ARG and _code(dec, run[:20]) == ARG
    assert _code(dec, run[:24]) == ARG
    for bad in (-1, 4):                                                     # idx_local outside 0 .. wK^2 - 1
        assert _code(dec, _set(run, 6 + per * 17, bad)) == ARG
    for bad in (-1, 8):                                                     # iso outside 0 .. 7
        assert _code(dec, _set(run, 6 + per * 17 + per - 1, bad)) == ARG
    assert _code(dec, _set(run, 4, 5)) == GEOM and _code(dec, _set(run, 4, 32)) == GEOM and _code(dec, _set(run, 1, 100)) == GEOM
    assert _code(dec, _set(run, 5, 0)) == WIN and _code(dec, _set(run, 5, 14)) == WIN
    for z in (0, 3, 8):
        assert _code(dec, run, zoom=z) == ARG
    # a short output: the zoomed size is reported
    L = capi.lib()
    fn, t = (L.fic_decode_gray_iso_run, C.c_uint8) if tag == 4 else (L.fic_decode_rgb_iso_run, C.c_int32)
    buf = np.frombuffer(run, np.uint8)
    out = np.zeros(256 * 128, np.uint8 if tag == 4 else np.int32)
    w, h = C.c_int(), C.c_int()
    assert fn(capi.ptr(buf, C.c_uint8), buf.size, 2, 0, capi.ptr(out, t), 256 * 128 - 1, C.byref(w), C.byref(h), None, None) == CAP
    assert (w.value, h.value) == (256, 128)


def test_quadtree_reader_refuses_malformed_streams(oracle):
    c = im.quadtree_case(*im.QT_CASES[1])
    run, lv = c["run"], c["leaves"]
    dec = fic_amd.decode_rgb_quadtree_iso_run
    for other in (0, 1, 2, 3, 4, 5, 7):
        assert _code(dec, _set(run, 0, other)) == ARG
    assert _code(dec, _set(run, 3, 16)) == ARG
    assert _code(dec, run[:-4]) == ARG and _code(dec, run + bytes(4)) == ARG and _code(dec, run[:28]) == ARG
    assert _code(dec, _set(run, 4, 32)) == ARG and _code(dec, _set(run, 5, 16)) == ARG and _code(dec, _set(run, 5, 2)) == ARG   # levels
    assert _code(dec, _set(run, 1, 120)) == GEOM                            # not a multiple of B_max
    assert _code(dec, _set(run, 6, -1)) == WIN and _code(dec, _set(run, 6, 0)) == WIN and _code(dec, _set(run, 6, 30)) == WIN
    assert _code(dec, _set(run, 7, 0)) == ARG and _code(dec, _set(run, 7, 128 * 64 // 16 + 1)) == ARG
    first16 = int(np.nonzero(lv[:, 2] == 16)[0][0])
    assert _code(dec, _set(run, 8 + 7 * first16, 8)) == ARG                 # sizes that do not tile
    assert _code(dec, _set(run, 8 + 7 * first16, 32)) == ARG
    for bad in (-1, 4):
        assert _code(dec, _set(run, 8 + 7 * 9 + 1, bad)) == ARG            # idx_local
    for bad in (-1, 8):
        assert _code(dec, _set(run, 8 + 7 * 9 + 6, bad)) == ARG            # iso
    for z in (0, 3):
        assert _code(dec, run, zoom=z) == ARG
    L = capi.lib()
    buf = np.frombuffer(run, np.uint8)
    out = np.zeros(512 * 256, np.int32)
    w, h = C.c_int(), C.c_int()
    assert L.fic_decode_rgb_quadtree_iso_run(capi.ptr(buf, C.c_uint8), buf.size, 4, 0, capi.ptr(out, C.c_int32), 512 * 256 - 1, C.byref(w),
                                             C.byref(h), None, None) == CAP
    assert (w.value, h.value) == (512, 256)


def test_the_older_readers_refuse_the_new_tags(oracle):
    """The 0 where a .run holds its block size: fic_decode_rgb_run refuses it as a geometry, fic_decode_gray_run refuses the
    non-zero tag, the quadtree readers refuse any tag but their own -- at every zoom."""
    runs = [im.fixed_case(4, 128, 64, 8, 2, 3)["run"], im.fixed_case(5, 128, 64, 8, 2, 3)["run"], im.quadtree_case(*im.QT_CASES[1])["run"]]
    for run in runs:
        for z in ZOOMS:
            assert _code(fic_amd.decode_rgb_run, run, zoom=z) == GEOM
            assert _code(fic_amd.decode_gray_run, run, zoom=z) == NOT_GREY
            assert _code(fic_amd.decode_quadtree_run, run, zoom=z) == ARG
            assert _code(fic_amd.decode_rgb_quadtree_run, run, zoom=z) == ARG
    # and the new readers refuse each other's and the older tags
    olds = [sm.fixed_case(0, 128, 64, 8, 2, 8)["run"], sm.fixed_case(1, 128, 64, 8, 2, 18)["run"],
            sm.grey_quadtree_case(*sm.QT_CASES[1])["run"], sm.rgb_quadtree_case(*sm.QT_CASES[1])["run"]]
    for i, dec in enumerate((fic_amd.decode_gray_iso_run, fic_amd.decode_rgb_iso_run, fic_amd.decode_rgb_quadtree_iso_run)):
        for run in olds + runs[:i] + runs[i + 1:]:
            assert _code(dec, run) == ARG


# ---- the model's identities -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,w,h,B,wK", [(4, 64, 64, 4, 0), (4, 128, 64, 16, 2), (5, 64, 64, 16, 0), (5, 128, 64, 8, 2)])
def test_fixed_streams_with_a_zero_column_decode_like_their_twins(oracle, tag, w, h, B, wK):
    c = im.fixed_case(tag, w, h, B, wK, 10 * (tag - 4) + B)
    twin = sm.fixed_case(tag - 4, w, h, B, wK, 10 * (tag - 4) + B)["run"]
    zero = im.write_fixed(tag, c["rows"], np.zeros_like(c["iso"]), w, h, B, c["wK"])
    for z in ZOOMS:
        assert _same(im.decode_fixed(zero, z), sm.reference(twin, z)), z
        assert not (im.reference(c["run"], z)[0] == sm.reference(twin, z)[0]).all(), z       # the isometries show
    assert _same(im.decode_fixed(zero, 2, 3.25), (zm.decode_gray if tag == 4 else zm.decode_rgb)(twin, 2, 3.25))


@pytest.mark.parametrize("w,h,wK,seed", im.QT_CASES[:3])
def test_quadtree_stream_with_a_zero_column_decodes_like_its_tag3_twin(oracle, w, h, wK, seed):
    c = im.quadtree_case(w, h, wK, seed)
    lv = c["leaves"].copy()
    lv[:, 8] = 0
    zero = im.write_qt(lv, w, h, 16, 4, wK)
    for z in ZOOMS:
        assert _same(im.decode_qt(zero, z), sm.reference(im.tag3_twin(zero), z)), z


@pytest.fixture(scope="module")
def crop(lena_colored, oracle):
    from oracle import fic_oracle as fo
    return fo.rgb_to_argb(np.ascontiguousarray(lena_colored[96:160, 64:128]))


def test_one_isometry_through_the_tag6_model_gives_the_colour_quadtree(crop):
    cbs = rm.codebooks(crop, 64, 64, 16, 4, 2)
    t, tree = zm.three_level_threshold(rm.level_sse(crop, 64, 64, cbs, 2), 64, 64)
    want = rm.encode(crop, 64, 64, 16, 4, 2, t, cbs)
    got = im.encode(crop, 64, 64, 16, 4, 2, 1, t)
    assert {int(b) for b in want[:, 2]} == {16, 8, 4}
    assert (got[:, :8] == want).all() and (got[:, 8] == 0).all()


def test_inf_threshold_stream_decodes_like_the_fixed_stream_in_the_model(crop):
    cbs = im.codebooks(crop, 64, 64, 16, 4, 2, 8)
    assert len(set(cbs[16][1].tolist())) >= 7                                # the encoder's own codebook exercises the isometries
    run6 = im.write_qt(im.encode(crop, 64, 64, 16, 4, 2, 8, float("inf"), cbs), 64, 64, 16, 4, 2)
    run5 = im.write_fixed(5, cbs[16][0], cbs[16][1], 64, 64, 16, 2)
    for z in ZOOMS:
        assert _same(im.decode_qt(run6, z), im.decode_fixed(run5, z)), z


@pytest.mark.parametrize("w,h,wK,seed", im.QT_CASES)
def test_every_isometry_shows_at_every_side_and_zoom(oracle, w, h, wK, seed):
    """Zero insensitive pairs: for every zoom z and every (z * side, k != 0) at least one leaf of that side and isometry holds a
    pixel that changes when the isometry column is zeroed (the definition of test_decode_streams_model.py for tag 2)."""
    c = im.quadtree_case(w, h, wK, seed)
    lv = c["leaves"].copy()
    lv[:, 8] = 0
    plain = im.write_qt(lv, w, h, 16, 4, wK)
    for z in ZOOMS:
        a, b = im.reference(c["run"], z)[0], im.decode_qt(plain, z)[0]
        seen = {(z * int(l[2]), int(l[8])) for l in c["leaves"] if l[8] and (_leaf(a, l, z) != _leaf(b, l, z)).any()}
        want = {(z * s, k) for s in (4, 8, 16) for k in range(1, 8)}
        assert seen == want, (z, sorted(want - seen))


def test_designated_rows_and_pool_corners_are_kept(oracle):
    for case in im.QT_CASES:
        c, t = im.quadtree_case(*case), sm.rgb_quadtree_case(*case)
        assert c["designated"] == t["designated"] and (c["leaves"][:, :8] == t["leaves"]).all()
        img = im.reference(c["run"], 1)[0]
        for (B, name), i in c["designated"].items():
            if name in sm.RGB_CONSTANT:                                      # a = 0: whatever the isometry
                assert (_leaf(img, c["leaves"][i], 1) == np.array(sm.RGB_CONSTANT[name])).all(), (B, name)


@pytest.mark.parametrize("name", ["tag4", "tag5", "tag6"])
def test_oscillators_run_50_iterations(oracle, name):
    run = im.oscillators()[name]
    (im.read_qt if name == "tag6" else im.read_fixed)(run)
    for z in (1, 4):
        img, avg, it = im.reference(run, z)
        assert it == 50 and avg >= 1, (name, z, avg)
        if z == 4:
            assert float(avg) * img.shape[0] * img.shape[1] >= 2 ** 24      # the float sum leaves the exact integers (FC:407)
