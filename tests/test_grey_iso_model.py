"""tests/greyisomodel.py against the oracle, on the CPU: the collage model equals fo_collage_gray at n_iso = 1; the oracle's
n_iso = 8 codebooks satisfy the painter-agreement inequality, with enough ranges that would break it if k = 1 and k = 3 were
exchanged between encoder and painter; a rotated image gets the rotated errors.  tests/test_gpu_collage.py holds the device to
the same model."""
import numpy as np
import pytest

import greyisomodel as gm
from conftest import same_f32


def _quadrants():
    """64 x 64: flat 90 | noise over flat 200 | noise -- flat range and domain blocks (NaN fits, rem = 0) beside busy ones."""
    g = np.random.RandomState(11).randint(0, 256, size=(64, 64)).astype(np.uint8)
    g[:32, :32] = 90
    g[32:, 32:] = 200
    return g


def _image(name, lena64, lena_grey):
    return {"lena64": lambda: lena64,
            "crop16": lambda: np.ascontiguousarray(lena_grey[64:192, 64:192]),
            "corner": lambda: np.ascontiguousarray(lena_grey[:128, :128]),
            "flat": lambda: np.full((64, 64), 77, np.uint8),
            "random": lambda: np.random.RandomState(5).randint(0, 256, size=(32, 48)).astype(np.uint8),
            "quadrants": _quadrants,
            "overshoot": gm.overshoot_image}[name]()


@pytest.mark.parametrize("name,B,wK", [("lena64", 4, 29), ("lena64", 4, 5), ("lena64", 8, 13), ("flat", 8, 13), ("random", 8, 2),
                                       ("random", 4, 3), ("quadrants", 8, 4), ("quadrants", 16, 5)])
def test_collage_model_is_the_oracles_collage(oracle, lena64, lena_grey, name, B, wK):
    g = _image(name, lena64, lena_grey)
    h, w = g.shape
    argb = oracle.gray_to_argb(g)
    ref = oracle.encode_gray(argb, w, h, B, wK, 1)
    info = ref["info"]
    got, v = gm.collage(g, B, gm.to_global(w, h, B, wK, info[:, 0]), info[:, 1], info[:, 2], ref["iso"])
    assert (got == oracle.collage_gray(argb, w, h, B, wK, info)).all()
    if name == "flat":                                                # every fit is 0 / 0: NaN paints 0
        assert np.isnan(v).all() and (got == np.int32(-16777216)).all()


@pytest.mark.parametrize("B,wK,below,above", [(4, 29, 24, 12), (4, 5, 32, 55), (8, 3, 16, 2), (8, 13, 0, 0)])
def test_overshoot_image_leaves_the_byte_range_on_both_sides(oracle, B, wK, below, above):
    """The clamp of the collage has work to do at B = 4 and at B = 8 with wK = 3, and none at B = 8 full search."""
    g = gm.overshoot_image()
    ref = oracle.encode_gray(oracle.gray_to_argb(g), 64, 64, B, wK, 8)
    info = ref["info"]
    _, v = gm.collage(g, B, gm.to_global(64, 64, B, wK, info[:, 0]), info[:, 1], info[:, 2], ref["iso"])
    assert (int((v < 0).sum()), int((v >= 256).sum())) == (below, above)


AGREEMENT = [("lena64", 4, 29, 232, 256, 41), ("lena64", 8, 13, 61, 64, 5), ("crop16", 16, 13, 64, 64, 5), ("corner", 8, 29, 248, 256, 30)]


def _agreement(oracle, g, B, wK):
    h, w = g.shape
    argb = oracle.gray_to_argb(g)
    ref = oracle.encode_gray(argb, w, h, B, wK, 8)
    gidx = gm.to_global(w, h, B, wK, ref["info"][:, 0])
    return gm.painter_agreement(g, B, oracle.pool(argb, w, h, B)[0], gidx, ref["info"][:, 1], ref["iso"])


@pytest.mark.parametrize("name,B,wK,used,total,strict13", AGREEMENT)
def test_oracle_codebooks_agree_with_the_painters(oracle, lena64, lena_grey, name, B, wK, used, total, strict13):
    c = _agreement(oracle, _image(name, lena64, lena_grey), B, wK)
    gm.check_agreement(c)
    assert (c["used"], c["total"], c["strict13"]) == (used, total, strict13)
    assert c["swapped_violations"] == strict13                        # exactly the ranges where dots[1] != dots[3] matters


@pytest.mark.parametrize("name,B,wK", [("lena64", 4, 29), ("crop16", 16, 13)])
def test_a_painter_that_exchanges_rotations_is_caught(oracle, lena64, lena_grey, monkeypatch, name, B, wK):
    """The model's own painter with cases 1 and 3 of the index map exchanged: the inequality breaks."""
    monkeypatch.setitem(gm._ISO, B, gm.iso_table(B)[[0, 3, 2, 1, 4, 5, 6, 7]])
    c = _agreement(oracle, _image(name, lena64, lena_grey), B, wK)
    assert c["violations"] >= 4


@pytest.mark.parametrize("size,B", [(64, 4), (64, 8), (128, 16)])
def test_rotated_image_gets_the_rotated_errors(oracle, size, B):
    """An image of 2 x 2 cells and its clockwise rotation, full search with the 8 isometries: the candidates of range block
    (bx, by) and those of its image (Rw - 1 - by, bx) are the same blocks up to an isometry, so the winning error has the same
    bits.  (All sums stay below 2^24, so their order does not show.)"""
    g = gm.cell_image(size, 17)
    r = np.ascontiguousarray(np.rot90(g, -1))
    Rw, _, Dw, _ = oracle.geometry(size, size, B)
    e = oracle.encode_gray(oracle.gray_to_argb(g), size, size, B, Dw, 8)["err"]
    er = oracle.encode_gray(oracle.gray_to_argb(r), size, size, B, Dw, 8)["err"]
    by, bx = np.divmod(np.arange(Rw * Rw), Rw)
    assert (e != 0).any()
    assert same_f32(er[(Rw - 1 - by) + bx * Rw], e)
