"""Quadtree (variable block size) grey codec, CPU side: the numpy model (tests/qtmodel.py) against the oracle's fixed-B
decoder, the tag-2 stream writer / reader of the library (host only) against the model, and the quality calibration that
the GPU tests rely on.  DESIGN.md section 4.13."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qtmodel as qm  # noqa: E402

import fic_amd  # noqa: E402
from fic_amd import capi  # noqa: E402

INF = float("inf")


@pytest.fixture(scope="module")
def lena_cbs(lena_grey, oracle):
    return qm.codebooks(lena_grey, 16, 4, 0, 1)


def _fixed_decode(oracle, gray, B, wK):
    h, w = gray.shape
    wk = qm.level_wk(w, h, B, wK)
    r = oracle.encode_gray(oracle.gray_to_argb(gray), w, h, B, wk, 1)
    return oracle.decode_gray(oracle.write_run_gray(r["info"], w, h, B, wk))


def _same_decode(a, b):
    return (a[0] == b[0]).all() and a[1].view(np.uint32) == b[1].view(np.uint32) and a[2] == b[2]


@pytest.mark.parametrize("B_max,B_min,wK", [(16, 4, 0), (8, 4, 0), (16, 8, 2), (8, 4, 3)])
def test_inf_threshold_decodes_like_fixed_bmax(lena64, oracle, B_max, B_min, wK):
    h, w = lena64.shape
    leaves = qm.encode(lena64, B_max, B_min, wK, 1, INF)
    assert (leaves[:, 2] == B_max).all() and len(leaves) == (w // B_max) * (h // B_max)
    got = qm.decode(qm.write_run(leaves, w, h, B_max, B_min, wK, 1))
    assert _same_decode(got, _fixed_decode(oracle, lena64, B_max, wK))


def test_inf_threshold_decodes_like_fixed_bmax_lena256(lena_grey, lena_cbs, oracle):
    h, w = lena_grey.shape
    leaves = qm.encode(lena_grey, 16, 4, 0, 1, INF, lena_cbs)
    got = qm.decode(qm.write_run(leaves, w, h, 16, 4, 0, 1))
    assert _same_decode(got, _fixed_decode(oracle, lena_grey, 16, 0))


def test_negative_threshold_gives_bmin_rows_in_dfs_order(lena64, oracle):
    h, w = lena64.shape
    cbs = qm.codebooks(lena64, 16, 4, 0, 8)
    leaves = qm.encode(lena64, 16, 4, 0, 8, -1.0, cbs)
    # DFS order of the 4x4 blocks inside every 16x16 block: Morton order of the 4x4 grid, blocks in scanline order
    morton = [(((i >> 0) & 1) | ((i >> 1) & 2), ((i >> 1) & 1) | ((i >> 2) & 2)) for i in range(16)]
    xy = [(bx * 16 + 4 * mx, by * 16 + 4 * my) for by in range(h // 16) for bx in range(w // 16) for mx, my in morton]
    assert [tuple(r[:2]) for r in leaves] == xy
    q, k = cbs[4]
    j = leaves[:, 1] // 4 * (w // 4) + leaves[:, 0] // 4
    assert (leaves[:, 3:6] == q[j]).all() and (leaves[:, 6] == k[j]).all()


def test_split_rule_is_strictly_greater(lena64):
    h, w = lena64.shape
    cbs = qm.codebooks(lena64, 16, 4, 0, 1)
    sse = qm.level_sse(lena64, cbs)
    s0 = int(sse[16][0, 0])
    # a threshold that makes SSE == threshold * B * B exactly does not split; one ulp below does
    t = np.float32(s0 / 256.0)
    if float(t) * 256.0 == s0:
        assert qm.split(sse, w, h, 16, 4, t)[0] == (0, 0, 16)
    below = np.nextafter(np.float32(s0 / 256.0), np.float32(-1))
    assert qm.split(sse, w, h, 16, 4, below)[0][2] < 16


def test_writer_matches_model_and_reader_round_trips(lena64):
    h, w = lena64.shape
    for n_iso, wK, t in ((1, 0, 300.0), (8, 2, 100.0)):
        leaves = qm.encode(lena64, 16, 4, wK, n_iso, t)
        assert len(set(leaves[:, 2])) > 1, "the threshold should give leaves of mixed size"
        run = capi.write_run_quadtree(leaves, w, h, 16, 4, wK, n_iso)
        assert run == qm.write_run(leaves, w, h, 16, 4, wK, n_iso)
        assert len(run) == 32 + 4 * (5 if n_iso == 8 else 4) * len(leaves)
        hd, back = qm.read_run(run)
        assert hd == dict(w=w, h=h, B_max=16, B_min=4, wK=wK, n_iso=n_iso)
        assert (back == leaves).all()


def _malformed(run, n_iso, first_B):
    per = 4 * (5 if n_iso == 8 else 4)
    b = bytearray(run)
    wrong_tiling = bytearray(b)
    # another level's size for the first leaf: the leaves' areas no longer add up to the image
    wrong_tiling[32:36] = (16 if first_B != 16 else 8).to_bytes(4, "big")
    bad_B = bytearray(b)
    bad_B[32:36] = (32).to_bytes(4, "big")
    bad_idx = bytearray(b)
    bad_idx[36:40] = (10 ** 6).to_bytes(4, "big")
    cases = {
        "tag0": bytes(b[:3]) + b"\x00" + bytes(b[4:]),
        "tag1": bytes(b[:3]) + b"\x01" + bytes(b[4:]),
        "truncated": bytes(b[:-4]),
        "one_leaf_short": bytes(b[:-per]),
        "oversized": bytes(b) + b"\x00\x00\x00\x00",
        "wrong_tiling": bytes(wrong_tiling),
        "B_outside_levels": bytes(bad_B),
        "bad_idx_local": bytes(bad_idx),
        "header_only": bytes(b[:32]),
    }
    return cases


@pytest.mark.parametrize("n_iso", [1, 8])
def test_reader_rejects_malformed_streams(lena64, n_iso):
    h, w = lena64.shape
    leaves = qm.encode(lena64, 16, 4, 0, n_iso, 200.0)
    run = qm.write_run(leaves, w, h, 16, 4, 0, n_iso)
    for name, bad in _malformed(run, n_iso, leaves[0, 2]).items():
        with pytest.raises(ValueError):
            qm.read_run(bad)
        # the library checks the stream before it looks for a device
        with pytest.raises(fic_amd.FicError) as e:
            capi.decode_quadtree_run(bad)
        assert e.value.code == -3, (name, str(e.value))


def test_writer_rejects_leaves_out_of_order(lena64):
    h, w = lena64.shape
    leaves = qm.encode(lena64, 16, 4, 0, 1, 200.0)
    swapped = leaves.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    with pytest.raises(fic_amd.FicError) as e:
        capi.write_run_quadtree(swapped, w, h, 16, 4, 0, 1)
    assert e.value.code == -3
    with pytest.raises(fic_amd.FicError):
        capi.write_run_quadtree(leaves[:-1], w, h, 16, 4, 0, 1)


@pytest.mark.parametrize("args,code", [
    ((16, 16, 0, 1, 0.0), -3),      # B_min == B_max
    ((4, 4, 0, 1, 0.0), -3),        # B_max = 4
    ((16, 2, 0, 1, 0.0), -3),       # B_min = 2
    ((16, 4, 0, 3, 0.0), -3),       # n_iso
    ((16, 4, 0, 1, float("nan")), -3),
    ((16, 4, -1, 1, 0.0), -2),
])
def test_encode_rejects_bad_arguments_before_the_device(lena64, args, code):
    B_max, B_min, wK, n_iso, t = args
    with pytest.raises(fic_amd.FicError) as e:
        capi.encode_gray_quadtree(lena64, B_max, B_min, wK, n_iso, t)
    assert e.value.code == code


def test_encode_rejects_non_multiple_of_bmax():
    with pytest.raises(fic_amd.FicError) as e:
        capi.encode_gray_quadtree(np.zeros((72, 72), np.uint8), 16, 4)
    assert e.value.code == -1


# Calibration on LenaGrey 256x256, 16 -> 4, full search, 1 isometry (model numbers):
#   threshold      leaves (4 / 8 / 16)      PSNR dB   iterations
#   +inf            256 (0 / 0 / 256)       22.068    7            = fixed B = 16
#   400             937 (564 / 203 / 170)   24.872    7
#   200            1291 (904 / 250 / 137)   25.732    7
#   100            1747 (1324 / 333 / 90)   26.507    7
# Fixed B = 8 (1024 rows) gives 24.8 dB, fixed B = 4 (4096 rows) 27.2 dB.
QT_THRESHOLD = 400.0
QT_LEAVES = 937


def test_quality_calibration_lena256(lena_grey, lena_cbs, oracle):
    h, w = lena_grey.shape
    leaves = qm.encode(lena_grey, 16, 4, 0, 1, QT_THRESHOLD, lena_cbs)
    assert len(leaves) == QT_LEAVES
    assert [int((leaves[:, 2] == B).sum()) for B in (4, 8, 16)] == [564, 203, 170]
    img, avg, it = qm.decode(qm.write_run(leaves, w, h, 16, 4, 0, 1))
    p = oracle.psnr(img, lena_grey)
    p16 = oracle.psnr(_fixed_decode(oracle, lena_grey, 16, 0)[0], lena_grey)
    assert abs(p - 24.872) < 5e-3 and abs(p16 - 22.068) < 5e-3
    assert p > p16 + 2.5
    assert len(leaves) < 4096 // 4
