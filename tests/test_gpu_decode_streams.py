"""The four decoders on the hand-built streams of tests/streammodel.py against the reference models,
exactly: pixels, alpha 0xFF for colour, avgError as a bit pattern, the iteration count.  What the streams cover -- every
isometry at the sides 4 .. 64 with every row segment, the pool's corner blocks, both sides of the clamp and Java's float-to-int
saturation in every channel, 50 iterations on the leaf-order squares, non-square images at zoom -- is asserted on the CPU by
tests/test_decode_streams_model.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qtrgbmodel as rm  # noqa: E402
import rgbisomodel as rim  # noqa: E402
import streammodel as sm  # noqa: E402
import zoommodel as zm  # noqa: E402

import fic_amd  # noqa: E402
from fic_amd import capi  # noqa: E402
from oracle import fic_oracle as fo  # noqa: E402

pytestmark = pytest.mark.gpu

ZOOMS = (1, 2, 4)
DECODERS = (fic_amd.decode_gray_run, fic_amd.decode_rgb_run, fic_amd.decode_quadtree_run, fic_amd.decode_rgb_quadtree_run)


def _bits(x):
    return int(np.float32(x).view(np.uint32))


def _same(got, want):
    """(pixels, avgError, iterations) of a grey decode, bit for bit."""
    return bool(got[0].shape == want[0].shape and (got[0] == want[0]).all() and _bits(got[1]) == _bits(want[1]) and got[2] == want[2])


def _same_rgb(argb, avg, it, want):
    """A GPU colour decode (packed ARGB of any shape) against a model's (rgb [h, w, 3], avgError, iterations)."""
    h, w = want[0].shape[:2]
    return bool(argb.size == w * h and (rm.channels(argb, w, h) == want[0]).all() and (argb.view(np.uint32) >> 24 == 0xFF).all()
                and _bits(avg) == _bits(want[1]) and it == want[2])


def _check(run, z, carry=0.0, what=None):
    """One stream of any tag through its decoder at zoom z against the reference; prints the figures before it asserts."""
    tag = run[3]
    got = DECODERS[tag](run, avg_error_in=carry, zoom=z)
    want = sm.reference(run, z, carry)
    print(f"{what} tag={tag} zoom={z} carry={carry}: iterations {got[2]} / {want[2]} avgError {got[1]!r} / {want[1]!r}")
    if tag in (1, 3):
        assert _same_rgb(got[0], got[1], got[2], want), (what, z, carry)
        if tag == 1:
            assert got[3:] == (want[0].shape[1], want[0].shape[0])
    else:
        assert _same(got, want), (what, z, carry, int((got[0] != want[0]).sum()) if got[0].shape == want[0].shape else got[0].shape)
    return want


@pytest.mark.parametrize("w,h,wK,seed", sm.QT_CASES)
def test_grey_quadtree_every_side_and_isometry(oracle, w, h, wK, seed):
    run = sm.grey_quadtree_case(w, h, wK, seed)["run"]
    for z in ZOOMS:
        _check(run, z, what=f"grey quadtree {w}x{h} wK={wK}")


@pytest.mark.parametrize("w,h,wK,seed", sm.QT_CASES)
def test_rgb_quadtree_clamps_and_pool_corners(oracle, w, h, wK, seed):
    run = sm.rgb_quadtree_case(w, h, wK, seed)["run"]
    for z in ZOOMS:
        _check(run, z, what=f"colour quadtree {w}x{h} wK={wK}")


@pytest.mark.parametrize("tag,w,h,B,wK,seed", sm.FIXED_CASES)
def test_fixed_block_streams(oracle, tag, w, h, B, wK, seed):
    run = sm.fixed_case(tag, w, h, B, wK, seed)["run"]
    for z in ZOOMS:
        _check(run, z, what=f"fixed B={B} {w}x{h} wK={wK}")


@pytest.mark.parametrize("B,size", [(4, 64), (8, 128), (16, 128)])
def test_rows_with_isometries_on_the_fixed_block_paint(oracle, B, size):
    """k_decode_paint's isometry branch is reached through a context only: the codebook of an image on which the n_iso = 8
    search chooses all 8 isometries, decoded at every zoom (sides up to 64, every segment) against the oracle's decoder."""
    img = sm.iso_tile_image(B, size)
    wk = capi.geometry(size, size, B)[2]
    with fic_amd.Encoder(size, size, B, None, 8) as enc:
        enc.set_gray(img)
        enc.encode()
        r = enc.results()
        assert set(r["iso"].reshape(-1).tolist()) == set(range(8))
        for z in ZOOMS:
            got = enc.decode(zoom=z)
            want = zm.decode_rows(r["qrows"][0], r["iso"][0], size, size, B, wk, z)
            print(f"rows B={B} zoom={z}: iterations {got[2][0]} / {want[2]} avgError {got[1][0]!r} / {want[1]!r}")
            assert _same((got[0][0], got[1][0], int(got[2][0])), want), (B, z)
    if B in (4, 16):
        argb = fo.rgb_to_argb(sm.iso_tile_image_rgb(B, size))
        with capi.RgbEncoder(size, size, B, wk, n_iso=8) as enc:
            enc.set_argb(argb)
            enc.encode()
            r = enc.results()
            assert set(r["iso"].reshape(-1).tolist()) == set(range(8))
            out, avg, it = enc.decode()
        want = rim.decode(r["qrows"][0], r["iso"][0], size, size, B, wk)
        assert _same_rgb(np.asarray(out[0]), avg[0], int(it[0]), want), B


def _decode_debug(run, w, h):
    buf = np.frombuffer(run, np.uint8)
    out = np.zeros(w * h, np.uint8)
    avg, it, seq = C.c_float(0.0), C.c_int(), C.c_int()
    capi.check(capi.lib().fic_debug_decode_gray_run(capi.ptr(buf, C.c_uint8), buf.size, 0, capi.ptr(out, C.c_uint8), out.size,
                                                    C.byref(avg), C.byref(it), C.byref(seq)))
    return out.reshape(h, w), np.float32(avg.value), it.value, seq.value


@pytest.mark.parametrize("name", sorted(sm.oscillators()))
def test_oscillating_streams_run_50_iterations(oracle, name):
    """a = -1 everywhere: no convergence, so the squares kept in Java's visiting order (block order for the fixed-B tags, leaf
    order e.sqoff + ry * B + x0 for the quadtree tags) are re-accumulated sequentially 50 times, at zoom 1 and in the row
    segments of zoom 4."""
    run = sm.oscillators()[name]
    for z in (1, 4):
        want = _check(run, z, what=name)
        assert want[2] == 50
    if name == "tag0":
        w, h = (int.from_bytes(run[o:o + 4], "big") for o in (4, 8))
        img, avg, it, seq = _decode_debug(run, w, h)
        assert seq > 0 and _same((img, avg, it), sm.reference(run, 1))


@pytest.mark.parametrize("carry", [0.75, 1.0e7])
def test_carry_in_on_hand_built_streams(oracle, carry):
    w, h, wK, seed = sm.QT_CASES[1]
    _check(sm.grey_quadtree_case(w, h, wK, seed)["run"], 4, carry, "grey quadtree carry")
    _check(sm.rgb_quadtree_case(w, h, wK, seed)["run"], 4, carry, "colour quadtree carry")
