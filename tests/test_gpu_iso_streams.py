"""Streams with an isometry column and the colour quadtree with the 8 isometries on the GPU against
tests/isostreammodel.py.  Every comparison is exact: pixels, avgError bits, iterations.  Fixed B (tags 4 and 5): the stream
decode against the decode of the context that made the codebook, against the model, and -- with the column zeroed -- against
the tag-0 / tag-1 decoder.  Colour quadtree (tag 6): per-level collage SSE, leaves, stream bytes and decode against the model,
+inf against the tag-5 stream, n_iso = 1 against the existing colour quadtree.  Hand-built streams with every (side, isometry)
pair (test_iso_streams_model.py shows that each pair changes pixels) and streams that never converge."""
import ctypes as C
import os
import sys
from functools import lru_cache

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
from oracle import fic_oracle as fo  # noqa: E402

pytestmark = pytest.mark.gpu

INF = float("inf")
ZOOMS = (1, 2, 4)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@lru_cache(maxsize=None)
def _crop(name):
    """(rgb uint8 [h, w, 3], argb int32 [h*w], w, h): the 64 x 64 crop of LenaColored on which an n_iso = 8 search picks every
    isometry at B = 16, 8 and 4, or the non-square 128 x 64 one beside it."""
    lena = np.load(os.path.join(GOLDEN, "lena_colored_256.npy"))
    rgb = np.ascontiguousarray(lena[96:160, 64:128] if name == "64" else lena[96:160, 64:192])
    h, w = rgb.shape[:2]
    return rgb, fo.rgb_to_argb(rgb), w, h


def _u32(x):
    return np.float32(x).view(np.uint32)


def _same_grey(got, want):
    return bool(got[0].shape == want[0].shape and (got[0] == want[0]).all() and _u32(got[1]) == _u32(want[1]) and got[2] == want[2])


def _same_rgb(got, want):
    """GPU colour decode (argb [h, w] or [h*w], avg, it, ...) against a model's (rgb [h, w, 3], avg, it): pixels, alpha 255,
    avgError bits, iterations."""
    h, w = want[0].shape[:2]
    a = np.asarray(got[0]).reshape(h, w)
    return bool((rm.channels(a, w, h) == want[0]).all() and (a.view(np.uint32) >> 24 == 0xFF).all()
                and _u32(got[1]) == _u32(want[1]) and got[2] == want[2])


def _same_gpu(a, b):
    """Two GPU decodes: pixels (any shape), avgError bits, iterations."""
    return bool((np.asarray(a[0]).reshape(-1) == np.asarray(b[0]).reshape(-1)).all() and _u32(a[1]) == _u32(b[1]) and a[2] == b[2])


# ---- fixed B: tags 4 and 5 --------------------------------------------------------------------------------------------------------
FIXED = [(c, "64", B, wK) for c in (False, True) for B in (4, 8, 16) for wK in (0, 2)] + [(False, "128x64", 8, 2), (True, "128x64", 16, 2)]


@pytest.mark.parametrize("colour,name,B,wK", FIXED)
def test_fixed_stream_decodes_like_its_context_the_model_and_its_twin(oracle, colour, name, B, wK):
    rgb, argb, w, h = _crop(name)
    wk = qm.level_wk(w, h, B, wK)
    if colour:
        with capi.RgbEncoder(w, h, B, wk, n_iso=8) as enc:
            enc.set_argb(argb)
            enc.encode()
            r = enc.results()
            ctx = {z: enc.decode(zoom=z) for z in ZOOMS}
        rows, iso = r["qrows"][0], r["iso"][0]
        run = fic_amd.write_run_rgb_iso(rows, iso, w, h, B, wk)
        zero = fic_amd.write_run_rgb_iso(rows, np.zeros_like(iso), w, h, B, wk)
        twin = fic_amd.write_run_rgb(rows, w, h, B, wk)
        dec, dec_twin, same = fic_amd.decode_rgb_iso_run, fic_amd.decode_rgb_run, _same_rgb
    else:
        with fic_amd.Encoder(w, h, B, wk, 8) as enc:
            enc.set_gray(np.ascontiguousarray(rgb[..., 0]))
            enc.encode()
            r = enc.results()
            ctx = {z: enc.decode(zoom=z) for z in ZOOMS}
        rows, iso = r["qrows"][0], r["iso"][0]
        run = fic_amd.write_run_gray_iso(rows, iso, w, h, B, wk)
        zero = fic_amd.write_run_gray_iso(rows, np.zeros_like(iso), w, h, B, wk)
        twin = fic_amd.write_run_gray(rows, w, h, B, wk)
        dec, dec_twin, same = fic_amd.decode_gray_iso_run, fic_amd.decode_gray_run, _same_grey
    assert run == im.write_fixed(5 if colour else 4, rows, iso, w, h, B, wk)
    # the encoder's own codebook exercises the isometries: seven or eight of them on the colour crop (rgbisomodel finds the same),
    # several on the others (the hand-built streams below hold every one at every side)
    assert len(set(iso.tolist())) >= (7 if colour and name == "64" else 3)
    for z in ZOOMS:
        got = dec(run, zoom=z)
        assert got[0].size == z * z * w * h
        assert _same_gpu(got, (ctx[z][0][0], ctx[z][1][0], ctx[z][2][0])), f"context decode at zoom {z}"
        assert same(got, im.reference(run, z)), f"model at zoom {z}"
        assert _same_gpu(dec(zero, zoom=z), dec_twin(twin, zoom=z)), f"zeroed column against the tag-{int(colour)} decoder at zoom {z}"
    assert same(dec(run, zoom=2, avg_error_in=3.25), im.decode_fixed(run, 2, 3.25))     # the carry-in convention


@pytest.mark.parametrize("n_iso", [1, 8])
def test_colour_context_decode_at_zoom(oracle, n_iso):
    """fic_rgb_ctx_decode_zoom_host: zoom = 1 is fic_rgb_ctx_decode_host bit for bit on both kinds of context; an n_iso = 1
    context at zoom 2 / 4 decodes like its tag-1 stream; a batch decodes plane by plane."""
    rgb, argb, w, h = _crop("64")
    L = capi.lib()
    with capi.RgbEncoder(w, h, 8, 2, planes=2, n_iso=n_iso) as enc:
        enc.set_argb(np.stack([argb, argb[::-1]]))
        enc.encode()
        rows = enc.results()["qrows"]
        plain = enc.decode()
        out, avg, it = np.zeros((2, w * h), np.int32), np.zeros(2, np.float32), np.zeros(2, np.int32)
        capi.check(L.fic_rgb_ctx_decode_zoom_host(enc._h, 1, capi.ptr(out, C.c_int32), capi.ptr(avg, C.c_float), capi.ptr(it, C.c_int)))
        assert (out == plain[0]).all() and (avg.view(np.uint32) == plain[1].view(np.uint32)).all() and (it == plain[2]).all()
        with pytest.raises(fic_amd.FicError) as e:
            enc.decode(zoom=3)
        assert e.value.code == -3
        if n_iso == 1:
            for z in (2, 4):
                got = enc.decode(zoom=z)
                for p in range(2):
                    want = fic_amd.decode_rgb_run(fic_amd.write_run_rgb(rows[p], w, h, 8, 2), zoom=z)
                    assert _same_gpu((got[0][p], got[1][p], got[2][p]), want), (z, p)


@pytest.mark.parametrize("tag,w,h,B,wK", [(t, w, h, B, wK) for t in (4, 5) for B in (4, 8, 16) for w, h, wK in ((64, 64, 0), (128, 64, 2))])
def test_hand_built_fixed_streams(oracle, tag, w, h, B, wK):
    """Every isometry in every block row and column, the saturation and clamp rows, the pool's corners."""
    c = im.fixed_case(tag, w, h, B, wK, 10 * (tag - 4) + B)
    dec, same = (fic_amd.decode_gray_iso_run, _same_grey) if tag == 4 else (fic_amd.decode_rgb_iso_run, _same_rgb)
    for z in ZOOMS:
        assert same(dec(c["run"], zoom=z), im.reference(c["run"], z)), z


# ---- colour quadtree: tag 6 ---------------------------------------------------------------------------------------------------------
QT = [("64", 16, 4, 0), ("64", 16, 4, 2), ("64", 8, 4, 0), ("64", 8, 4, 2), ("128x64", 16, 4, 2)]


@pytest.mark.parametrize("name,B_max,B_min,wK", QT)
def test_colour_quadtree_with_isometries_matches_model(oracle, name, B_max, B_min, wK):
    _, argb, w, h = _crop(name)
    cbs = im.codebooks(argb, w, h, B_max, B_min, wK, 8)
    sse = im.level_sse(argb, w, h, cbs, wK)
    got = capi.debug_rgb_quadtree_iso_sse(argb, w, h, B_max, B_min, wK, 8)
    for B in qm.levels(B_max, B_min):
        assert (got[B].astype(np.int64) == sse[B]).all(), f"SSE at B={B}"
        assert len(set(cbs[B][1].tolist())) >= (7 if name == "64" else 4)
    t3, tree3 = zm.three_level_threshold(sse, w, h, B_max, B_min)
    assert {b for _, _, b in tree3} == set(qm.levels(B_max, B_min))         # leaves of every side occur
    for t in (INF, -1.0, t3):
        leaves = fic_amd.encode_rgb_quadtree_iso(argb, w, h, B_max, B_min, wK, 8, t)
        want = im.leaf_table(qm.split(sse, w, h, B_max, B_min, t), cbs, w)
        assert leaves.shape == want.shape and (leaves == want).all(), f"leaf table at threshold {t}"
        run = fic_amd.write_run_rgb_quadtree_iso(leaves, w, h, B_max, B_min, wK)
        assert run == im.write_qt(want, w, h, B_max, B_min, wK)
        if t == INF:          # the fixed-B_max rows of encode_rgb(n_iso = 8) in scanline order; the tag-5 stream decodes alike
            wk = qm.level_wk(w, h, B_max, wK)
            r = capi.encode_rgb(argb, w, h, B_max, wk, n_iso=8)
            assert (leaves[:, 2] == B_max).all() and (leaves[:, 3:8] == r["qrows"]).all() and (leaves[:, 8] == r["iso"]).all()
            run5 = fic_amd.write_run_rgb_iso(r["qrows"], r["iso"], w, h, B_max, wk)
            for z in ZOOMS:
                assert _same_gpu(fic_amd.decode_rgb_quadtree_iso_run(run, zoom=z), fic_amd.decode_rgb_iso_run(run5, zoom=z)), z
        if t < 0:             # every B_min block, depth first
            j = leaves[:, 1] // B_min * (w // B_min) + leaves[:, 0] // B_min
            assert (leaves[:, 2] == B_min).all() and (np.sort(j) == np.arange((w // B_min) * (h // B_min))).all()
        for z in ZOOMS:
            assert _same_rgb(fic_amd.decode_rgb_quadtree_iso_run(run, zoom=z), im.reference(run, z)), f"decode at threshold {t}, zoom {z}"


@pytest.mark.parametrize("name,B_max,B_min,wK", [("64", 16, 4, 0), ("128x64", 8, 4, 2)])
def test_one_isometry_is_the_existing_colour_quadtree(oracle, name, B_max, B_min, wK):
    _, argb, w, h = _crop(name)
    old_sse = capi.debug_rgb_quadtree_sse(argb, w, h, B_max, B_min, wK)
    new_sse = capi.debug_rgb_quadtree_iso_sse(argb, w, h, B_max, B_min, wK, 1)
    t3, _ = zm.three_level_threshold({B: v.astype(np.int64) for B, v in old_sse.items()}, w, h, B_max, B_min)
    for B in old_sse:
        assert (old_sse[B] == new_sse[B]).all()
    for t in (INF, t3, -1.0):
        old = fic_amd.encode_rgb_quadtree(argb, w, h, B_max, B_min, wK, t)
        new = fic_amd.encode_rgb_quadtree_iso(argb, w, h, B_max, B_min, wK, 1, t)
        assert (new[:, :8] == old).all() and (new[:, 8] == 0).all()
        run3 = fic_amd.write_run_rgb_quadtree(old, w, h, B_max, B_min, wK)
        run6 = fic_amd.write_run_rgb_quadtree_iso(new, w, h, B_max, B_min, wK)
        assert im.tag3_twin(run6) == run3
        for z in (ZOOMS if t == t3 else (1,)):
            assert _same_gpu(fic_amd.decode_rgb_quadtree_iso_run(run6, zoom=z), fic_amd.decode_rgb_quadtree_run(run3, zoom=z)), (t, z)


def test_encode_refuses_what_the_colour_quadtree_refuses(oracle):
    _, argb, w, h = _crop("64")
    E = fic_amd.encode_rgb_quadtree_iso
    for bad, code in ((dict(n_iso=2), -3), (dict(n_iso=0), -3), (dict(B_max=32), -3), (dict(B_min=16), -3), (dict(wK=-1), -2),
                      (dict(wK=14), -2), (dict(threshold=float("nan")), -3)):
        a = dict(B_max=16, B_min=4, wK=2, n_iso=8, threshold=INF)
        a.update(bad)
        with pytest.raises(fic_amd.FicError) as e:
            E(argb, w, h, a["B_max"], a["B_min"], a["wK"], a["n_iso"], a["threshold"])
        assert e.value.code == code, bad
    with pytest.raises(fic_amd.FicError) as e:
        E(argb[:w * 56], w, 56, 16, 4, 2)                                    # not a multiple of B_max
    assert e.value.code == -1


@pytest.mark.parametrize("z", ZOOMS)
@pytest.mark.parametrize("w,h,wK,seed", im.QT_CASES)
def test_hand_built_quadtree_streams(oracle, w, h, wK, seed, z):
    """Every (side, isometry) pair at sides 4 .. 64, the saturation and clamp rows of streammodel.RGB_ROWS, the pool-corner
    leaves; with the column zeroed, the tag-3 decoder's bits."""
    c = im.quadtree_case(w, h, wK, seed)
    got = fic_amd.decode_rgb_quadtree_iso_run(c["run"], zoom=z)
    assert got[0].shape == (z * h, z * w)
    assert _same_rgb(got, im.reference(c["run"], z))
    lv = c["leaves"].copy()
    lv[:, 8] = 0
    zero = im.write_qt(lv, w, h, 16, 4, wK)
    plain = fic_amd.decode_rgb_quadtree_run(im.tag3_twin(zero), zoom=z)
    assert _same_gpu(fic_amd.decode_rgb_quadtree_iso_run(zero, zoom=z), plain)
    assert not (got[0] == plain[0]).all()


@pytest.mark.parametrize("z", [1, 4])
@pytest.mark.parametrize("name", ["tag4", "tag5", "tag6"])
def test_streams_that_never_converge(oracle, name, z):
    """a = -1 everywhere: 50 iterations, avgError >= 1, and at zoom 4 every iteration's sum of squares is beyond 2^24, so the
    squares kept in Java's visiting order are re-accumulated sequentially."""
    run = im.oscillators()[name]
    dec, same = {"tag4": (fic_amd.decode_gray_iso_run, _same_grey), "tag5": (fic_amd.decode_rgb_iso_run, _same_rgb),
                 "tag6": (fic_amd.decode_rgb_quadtree_iso_run, _same_rgb)}[name]
    got, want = dec(run, zoom=z), im.reference(run, z)
    assert same(got, want)
    assert got[2] == 50 and got[1] >= 1
    if z == 4:
        assert float(got[1]) * got[0].size >= 2 ** 24
