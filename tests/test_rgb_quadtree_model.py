"""Quadtree (variable block size) joint-RGB codec, CPU side: the numpy model (tests/qtrgbmodel.py) against the oracle's
decodeRGB, the tag-3 stream writer / reader of the library (host only) against the model, the checks every entry makes before
it looks for a device, and the quality calibration that the GPU tests rely on.  DESIGN.md section 4.14."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qtrgbmodel as rm  # noqa: E402

import fic_amd  # noqa: E402
from fic_amd import capi  # noqa: E402

INF = float("inf")

# Calibration on LenaColored 256x256, 16 -> 4, full search (model numbers; threshold in decodeRGB's avgError unit, the squared
# error per pixel summed over R, G, B):
#   threshold      leaves (4 / 8 / 16)        PSNR dB   iterations
#   +inf            256 (0 / 0 / 256)         18.531    13           = fixed B = 16
#   2400           1111 (744 / 210 / 157)     19.989    13
#   1200           1759 (1356 / 309 / 94)     21.521    14
#   600            2332 (1956 / 323 / 53)     21.795    14
# Fixed B = 8 (1024 rows) gives 20.111 dB, fixed B = 4 (4096 rows) 21.811 dB.
QT_THRESHOLD = 1200.0
QT_LEAVES = 1759
QT_LEAVES_PER_B = [1356, 309, 94]
QT_PSNR = 21.521
CALIBRATION = {INF: (256, [0, 0, 256], 18.531, 13), 2400.0: (1111, [744, 210, 157], 19.989, 13),
               QT_THRESHOLD: (QT_LEAVES, QT_LEAVES_PER_B, QT_PSNR, 14), 600.0: (2332, [1956, 323, 53], 21.795, 14)}


def _argb(rgb):
    from oracle import fic_oracle as fo
    h, w = rgb.shape[:2]
    return fo.rgb_to_argb(np.ascontiguousarray(rgb)), w, h


def _same_decode(a, b):
    return bool((a[0] == b[0]).all() and a[1].view(np.uint32) == b[1].view(np.uint32) and a[2] == b[2])


@pytest.fixture(scope="module")
def lena_cbs(lena_colored, oracle):
    argb, w, h = _argb(lena_colored)
    return rm.codebooks(argb, w, h, 16, 4, 0)


@pytest.mark.parametrize("crop,B_max,wK", [((64, 64), 16, 0), ((64, 64), 8, 2), ((64, 128), 16, 2), ((256, 256), 16, 0),
                                           ((256, 256), 8, 0), ((256, 256), 16, 2), ((256, 256), 8, 2)])
def test_inf_threshold_decodes_like_fixed_bmax(lena_colored, oracle, crop, B_max, wK):
    """At +inf the leaves are the fixed-B_max rows; the tag-3 stream decodes like the oracle's decodeRGB of the .run.  The
    64x128 crop (W > H) takes scaleImageRGB's `x + 1 >= height` branch."""
    argb, w, h = _argb(lena_colored[:crop[0], :crop[1]])
    cbs = rm.codebooks(argb, w, h, B_max, 4, wK, only=(B_max,))
    leaves = rm.encode(argb, w, h, B_max, 4, wK, INF, cbs)
    assert (leaves[:, 2] == B_max).all() and len(leaves) == (w // B_max) * (h // B_max)
    got = rm.decode(rm.write_run(leaves, w, h, B_max, 4, wK))
    wk = rm.level_wk(w, h, B_max, wK)
    want = oracle.decode_rgb(oracle.write_run_rgb(oracle.encode_rgb(argb, w, h, B_max, wk), w, h, B_max, wk))
    assert _same_decode(got, want)


def test_scale_rgb_quirks():
    img = np.zeros((4, 6, 3), np.int64)
    img[1, 0] = (4, 8, 12)          # (x, y+1) of the first 2x2 cell: counted twice
    img[1, 1] = (100, 100, 100)     # (x+1, y+1): never counted
    img[1, 4] = (40, 40, 40)        # x + 1 >= height (5 >= 4): the fourth tap is 128
    s = rm.scale_rgb(img)
    assert (s[0, 0] == (2, 4, 6)).all()
    assert (s[0, 2] == (42, 42, 42)).all()          # (0 + 0 + 40 + 128) / 4


def test_threshold_extremes(lena_colored, oracle):
    argb, w, h = _argb(lena_colored[64:128, 64:128])
    cbs = rm.codebooks(argb, w, h, 16, 4, 0)
    neg = rm.encode(argb, w, h, 16, 4, 0, -1.0, cbs)
    # DFS order of the 4x4 blocks inside every 16x16 block: Morton order of the 4x4 grid, blocks in scanline order
    morton = [(((i >> 0) & 1) | ((i >> 1) & 2), ((i >> 1) & 1) | ((i >> 2) & 2)) for i in range(16)]
    xy = [(bx * 16 + 4 * mx, by * 16 + 4 * my) for by in range(h // 16) for bx in range(w // 16) for mx, my in morton]
    assert (neg[:, 2] == 4).all() and [tuple(r[:2]) for r in neg] == xy
    j = neg[:, 1] // 4 * (w // 4) + neg[:, 0] // 4
    assert (neg[:, 3:] == cbs[4][j]).all()
    inf = rm.encode(argb, w, h, 16, 4, 0, INF, cbs)
    assert (inf[:, 2] == 16).all() and (inf[:, 3:] == cbs[16]).all()


def test_writer_matches_model_and_reader_round_trips(lena_colored, oracle):
    argb, w, h = _argb(lena_colored[:64, :128])
    for wK, t in ((2, 600.0), (3, 300.0)):
        leaves = rm.encode(argb, w, h, 16, 4, wK, t)
        assert len(set(leaves[:, 2])) > 1, "the threshold should give leaves of mixed size"
        run = capi.write_run_rgb_quadtree(leaves, w, h, 16, 4, wK)
        assert run == rm.write_run(leaves, w, h, 16, 4, wK)
        assert len(run) == 32 + 24 * len(leaves)
        hd, back = rm.read_run(run)
        assert hd == dict(w=w, h=h, B_max=16, B_min=4, wK=wK)
        assert (back == leaves).all()
        # decoding the model's stream converges like decodeRGB does
        img, avg, it = rm.decode(run)
        assert avg < 1 and it < 50


def _malformed(run, first_B):
    b = bytes(run)

    def put(off, v):
        x = bytearray(b)
        x[off:off + 4] = int(v).to_bytes(4, "big", signed=True)
        return bytes(x)

    return {
        "tag0": put(0, 0), "tag1": put(0, 1), "tag2": put(0, 2),
        "fourth_int_not_zero": put(12, 8),
        "B_min_equals_B_max": put(20, 16), "B_max_4": put(16, 4),
        "w_not_multiple": put(4, 72),
        "wK_0_non_square": put(4, 128),
        "truncated": b[:-4], "one_leaf_short": b[:-24], "oversized": b + b"\0\0\0\0", "header_only": b[:32],
        "n_leaves_0": put(28, 0), "n_leaves_too_many": put(28, 10 ** 6),
        "wrong_tiling": put(32, 16 if first_B != 16 else 8),
        "B_outside_levels": put(32, 32),
        "bad_idx_local": put(36, 10 ** 6), "negative_idx_local": put(36, -1),
    }


def test_reader_rejects_malformed_streams(lena_colored, oracle):
    argb, w, h = _argb(lena_colored[:64, :64])
    leaves = rm.encode(argb, w, h, 16, 4, 0, 600.0)
    run = rm.write_run(leaves, w, h, 16, 4, 0)
    rm.read_run(run)
    for name, bad in _malformed(run, leaves[0, 2]).items():
        with pytest.raises(ValueError):
            rm.read_run(bad)
        # the library checks the stream before it looks for a device
        with pytest.raises(fic_amd.FicError) as e:
            capi.decode_rgb_quadtree_run(bad)
        assert e.value.code == -3, (name, str(e.value))


def test_existing_readers_refuse_tag3(lena_colored, oracle):
    argb, w, h = _argb(lena_colored[:64, :64])
    run = rm.write_run(rm.encode(argb, w, h, 16, 4, 0, 600.0), w, h, 16, 4, 0)
    for fn, code in ((capi.decode_gray_run, -6), (capi.decode_rgb_run, -1), (capi.decode_quadtree_run, -3)):
        with pytest.raises(fic_amd.FicError) as e:
            fn(run)
        assert e.value.code == code, fn.__name__


def test_writer_rejects_leaves_out_of_order(lena_colored, oracle):
    argb, w, h = _argb(lena_colored[:64, :64])
    leaves = rm.encode(argb, w, h, 16, 4, 0, 600.0)
    swapped = leaves.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    with pytest.raises(fic_amd.FicError) as e:
        capi.write_run_rgb_quadtree(swapped, w, h, 16, 4, 0)
    assert e.value.code == -3
    with pytest.raises(fic_amd.FicError):
        capi.write_run_rgb_quadtree(leaves[:-1], w, h, 16, 4, 0)


@pytest.mark.parametrize("args,code", [
    ((16, 16, 0, 0.0), -3),      # B_min == B_max
    ((4, 4, 0, 0.0), -3),        # B_max = 4
    ((16, 2, 0, 0.0), -3),       # B_min = 2
    ((16, 4, 0, float("nan")), -3),
    ((16, 4, -1, 0.0), -2),
])
def test_encode_rejects_bad_arguments_before_the_device(args, code):
    B_max, B_min, wK, t = args
    with pytest.raises(fic_amd.FicError) as e:
        capi.encode_rgb_quadtree(np.zeros(64 * 64, np.int32), 64, 64, B_max, B_min, wK, t)
    assert e.value.code == code


def test_encode_rejects_bad_geometry_before_the_device():
    with pytest.raises(fic_amd.FicError) as e:
        capi.encode_rgb_quadtree(np.zeros(72 * 72, np.int32), 72, 72, 16, 4)
    assert e.value.code == -1
    with pytest.raises(fic_amd.FicError) as e:            # wK = 0 needs a square image
        capi.encode_rgb_quadtree(np.zeros(64 * 128, np.int32), 128, 64, 16, 4, 0)
    assert e.value.code == -2


def test_quality_calibration_lena256(lena_colored, lena_cbs, oracle):
    argb, w, h = _argb(lena_colored)
    sse = rm.level_sse(argb, w, h, lena_cbs, 0)
    for t, (n, per_B, psnr, iters) in CALIBRATION.items():
        leaves = rm.leaf_table(rm.split(sse, w, h, 16, 4, t), lena_cbs, w)
        assert len(leaves) == n and [int((leaves[:, 2] == B).sum()) for B in (4, 8, 16)] == per_B, t
        img, avg, it = rm.decode(rm.write_run(leaves, w, h, 16, 4, 0))
        assert abs(oracle.psnr(img, lena_colored) - psnr) < 5e-3 and it == iters, t
