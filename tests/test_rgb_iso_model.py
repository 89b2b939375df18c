"""The numpy model of the joint-RGB codec with isometries (tests/rgbisomodel.py) against the unchanged
oracle: with n_iso = 1 it is fo_encode_rgb / fo_collage_rgb / fo_decode_rgb bit for bit (and unknown.run byte for byte); with
n_iso = 8 it never does worse, and on a rotated image the rotated range blocks pick the rotated answer.  CPU only."""
import os

import numpy as np
import pytest

import rgbisomodel as rm
from conftest import GOLDEN, same_f32


def _crop(lena_colored, size, x0=64, y0=96):
    return np.ascontiguousarray(lena_colored[y0:y0 + size, x0:x0 + size])


def _same_as_oracle(oracle, rgb, B, wK):
    h, w = rgb.shape[:2]
    argb = oracle.rgb_to_argb(rgb)
    ref = oracle.encode_rgb(argb, w, h, B, wK)
    got = rm.encode(argb, w, h, B, wK, 1)
    assert same_f32(got["info"], ref)
    assert (got["iso"] == 0).all()
    assert (got["qrows"] == oracle.quantise_rgb(ref)).all()
    assert (rm.collage(argb, w, h, B, wK, got["info"], got["iso"]) == oracle.collage_rgb(argb, w, h, B, wK, ref)).all()
    img, avg, it = rm.decode(got["qrows"], got["iso"], w, h, B, wK)
    rimg, ravg, rit = oracle.decode_rgb(oracle.write_run_rgb(ref, w, h, B, wK))
    assert (img == rimg).all()
    assert same_f32(avg, ravg) and it == rit


@pytest.mark.parametrize("B,wK", [(4, 2), (4, 29), (8, 4), (8, 13), (16, 2), (16, 5)])
def test_one_isometry_is_the_oracle_lena_64(lena_colored, oracle, B, wK):
    _same_as_oracle(oracle, _crop(lena_colored, 64), B, wK)


@pytest.mark.parametrize("B,wK", [(8, 8), (16, 13), (4, 4)])
def test_one_isometry_is_the_oracle_lena_128(lena_colored, oracle, B, wK):
    _same_as_oracle(oracle, _crop(lena_colored, 128), B, wK)


def test_one_isometry_reproduces_unknown_run(lena_colored, oracle):
    """unknown.run's geometry: LenaColored 256 x 256, B = 8, wK = 2."""
    argb = oracle.rgb_to_argb(lena_colored)
    got = rm.encode(argb, 256, 256, 8, 2, 1)
    assert oracle.write_run_rgb(got["info"], 256, 256, 8, 2) == open(os.path.join(GOLDEN, "unknown_run.bin"), "rb").read()


@pytest.mark.parametrize("size,B,wK", [(64, 4, 29), (64, 8, 13), (64, 8, 2), (128, 16, 4), (128, 8, 8)])
def test_eight_isometries_never_lose(lena_colored, oracle, size, B, wK):
    """k = 0 of every candidate is the n_iso = 1 candidate with the same arithmetic, so the n_iso = 8 winner's error is never above
    the n_iso = 1 winner's; where the two agree on (c, 0) the rows agree bit for bit."""
    rgb = _crop(lena_colored, size)
    argb = oracle.rgb_to_argb(rgb)
    one = rm.encode(argb, size, size, B, wK, 1)
    eight = rm.encode(argb, size, size, B, wK, 8)
    assert (eight["err"] <= one["err"]).all()
    assert (eight["iso"] >= 0).all() and (eight["iso"] < 8).all() and (eight["iso"] != 0).any()
    same = (eight["iso"] == 0) & (eight["info"][:, 0] == one["info"][:, 0])
    assert same.any() and same_f32(eight["info"][same], one["info"][same])
    assert (eight["err"] < one["err"]).any()


def _cells(size, seed):
    """Colour image of 2 x 2 constant cells: scaleImageRGB returns the cell values whatever its taps, so the scaled image -- and
    with it the pool -- of the rotated image is the rotation of the original's."""
    rng = np.random.RandomState(seed)
    c = rng.randint(90, 161, size=(size // 2, size // 2, 3))
    return np.repeat(np.repeat(c, 2, axis=0), 2, axis=1).astype(np.uint8)


@pytest.mark.parametrize("B", [4, 8])
def test_rotated_image_picks_the_rotated_answer(oracle, B):
    """Rotate the image by 90 degrees clockwise.  Range block j' of the rotated image is the rotation of range block j, the pool
    the rotation of the pool, and the set {D_k} of a domain block is closed under rotation: every (candidate, isometry) error
    of j' is one of j (all sums stay below 2^24 here -- |grey| <= 213, n <= 64 -- so the accumulation order does not round).
    So the winning error is the same bit pattern, and where j has no exact tie for it, what j' is painted from is the rotation
    of what j is painted from."""
    S = 64
    rgb = _cells(S, 5 + B)
    rot = np.ascontiguousarray(np.rot90(rgb, -1))                     # clockwise
    Dw = oracle.geometry(S, S, B)[2]
    a0, a1 = oracle.rgb_to_argb(rgb), oracle.rgb_to_argb(rot)
    e0, e1 = rm.encode(a0, S, S, B, Dw, 8), rm.encode(a1, S, S, B, Dw, 8)
    Rw = S // B
    j = np.arange(Rw * Rw)
    jy, jx = j // Rw, j % Rw
    jrot = jx * Rw + (Rw - 1 - jy)                                    # block (jx, jy) lands at (Rw-1-jy, jx)
    assert same_f32(e1["err"][jrot], e0["err"])

    def painted(argb, e):
        import qtrgbmodel as qr
        d = rm._domain_pixels(qr.scale_rgb(qr.channels(argb, S, S)), S, S, B, Dw, e["info"][:, 0].astype(np.int32), e["iso"])
        return d.reshape(-1, B, B, 3)

    p0, p1 = painted(a0, e0), painted(a1, e1)
    _, vR = oracle.range_rgb(a0, S, S, B)
    live = vR != 0                                                    # varianzRange = 0: every candidate ties at error 0
    assert live.sum() > len(j) // 2
    want = np.rot90(p0, -1, axes=(1, 2))
    assert (p1[jrot][live] == want[live]).all()
    assert (e1["iso"][jrot][live] != e0["iso"][live]).any()           # the answer moved with the image
