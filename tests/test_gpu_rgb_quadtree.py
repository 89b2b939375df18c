"""Quadtree (variable block size) joint-RGB codec on the GPU against the numpy model (tests/qtrgbmodel.py): per-level collage
SSE, the leaf table for several thresholds, the tag-3 stream and the decoder (pixels, avgError bits, iterations).  The model
runs on the GPU's own one-shot RGB codebooks (encode_rgb), which the quadtree encode must reproduce level by level.
DESIGN.md section 4.14."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qtrgbmodel as rm  # noqa: E402
from test_rgb_quadtree_model import QT_LEAVES, QT_LEAVES_PER_B, QT_PSNR, QT_THRESHOLD  # noqa: E402

import fic_amd  # noqa: E402
from fic_amd import capi, synth  # noqa: E402
from oracle import fic_oracle as fo  # noqa: E402

pytestmark = pytest.mark.gpu

INF = float("inf")
THRESHOLDS = (INF, 1200.0, 200.0, 0.0, -1.0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _image(name):
    """(argb int32 [h*w], w, h): LenaColored 256x256, or three synth planes of kind U / S, "<kind><w>x<h>" or "<kind><n>"."""
    if name == "lena256":
        rgb = np.load(os.path.join(GOLDEN, "lena_colored_256.npy"))
    else:
        kind, dims = name[0], name[1:].split("x")
        w = int(dims[0])
        h = int(dims[-1])
        seed = synth.SEEDS["cfg5"] + w + 7 * h
        rgb = np.stack([synth.image(kind, w, h, seed + c) for c in range(3)], axis=-1)
    h, w = rgb.shape[:2]
    return fo.rgb_to_argb(rgb), w, h


def _gpu_codebooks(argb, w, h, B_max, B_min, wK):
    return {B: capi.encode_rgb(argb, w, h, B, rm.level_wk(w, h, B, wK))["qrows"] for B in rm.levels(B_max, B_min)}


def _same_decode(got, want):
    """GPU decode (argb [h, w], avg, it) against the model's (rgb [h, w, 3], avg, it): pixels, alpha 255, avgError bits."""
    h, w = got[0].shape
    return bool((rm.channels(got[0], w, h) == want[0]).all() and (got[0].view(np.uint32) >> 24 == 0xFF).all()
                and got[1].view(np.uint32) == want[1].view(np.uint32) and got[2] == want[2])


CASES = [
    ("U64", 16, 4, 0), ("S64", 16, 8, 2), ("U128", 8, 4, 2), ("S128", 16, 4, 0),
    ("lena256", 16, 4, 0), ("S192x128", 16, 4, 2),
]


@pytest.mark.parametrize("name,B_max,B_min,wK", CASES)
def test_rgb_quadtree_matches_model(name, B_max, B_min, wK):
    argb, w, h = _image(name)
    cbs = _gpu_codebooks(argb, w, h, B_max, B_min, wK)
    sse = rm.level_sse(argb, w, h, cbs, wK)
    got = capi.debug_rgb_quadtree_sse(argb, w, h, B_max, B_min, wK)
    for B in rm.levels(B_max, B_min):
        assert (got[B].astype(np.int64) == sse[B]).all(), f"SSE at B={B}"
    for t in THRESHOLDS:
        leaves = fic_amd.encode_rgb_quadtree(argb, w, h, B_max, B_min, wK, t)
        want = rm.leaf_table(rm.split(sse, w, h, B_max, B_min, t), cbs, w)
        assert leaves.shape == want.shape and (leaves == want).all(), f"leaf table at threshold {t}"
        if t == INF:          # the fixed-B_max rows of encode_rgb in scanline order
            assert (leaves[:, 2] == B_max).all() and (leaves[:, 3:] == cbs[B_max]).all()
        if t < 0:             # every B_min row of encode_rgb, depth first
            j = leaves[:, 1] // B_min * (w // B_min) + leaves[:, 0] // B_min
            assert (leaves[:, 2] == B_min).all() and (np.sort(j) == np.arange((w // B_min) * (h // B_min))).all()
            assert (leaves[:, 3:] == cbs[B_min][j]).all()
        if t in (INF, 200.0, -1.0):
            run = fic_amd.write_run_rgb_quadtree(leaves, w, h, B_max, B_min, wK)
            assert run == rm.write_run(want, w, h, B_max, B_min, wK)
            dec = fic_amd.decode_rgb_quadtree_run(run)
            assert _same_decode(dec, rm.decode(run)), f"decode at threshold {t}"
            if t == INF:      # the fixed-B_max .run of the same codebook decodes to the same bits
                wk = rm.level_wk(w, h, B_max, wK)
                fixed = fic_amd.decode_rgb_run(fic_amd.write_run_rgb(cbs[B_max], w, h, B_max, wk))
                assert (dec[0].reshape(-1) == fixed[0]).all() and dec[1].view(np.uint32) == fixed[1].view(np.uint32)
                assert dec[2] == fixed[2]


def test_calibration_and_avg_error_carry():
    argb, w, h = _image("lena256")
    leaves = fic_amd.encode_rgb_quadtree(argb, w, h, 16, 4, 0, QT_THRESHOLD)
    assert len(leaves) == QT_LEAVES                     # the CPU calibration (test_rgb_quadtree_model)
    assert [int((leaves[:, 2] == B).sum()) for B in (4, 8, 16)] == QT_LEAVES_PER_B
    run = fic_amd.write_run_rgb_quadtree(leaves, w, h, 16, 4, 0)
    img, avg, it = fic_amd.decode_rgb_quadtree_run(run)
    assert abs(fo.psnr(rm.channels(img, w, h), rm.channels(argb, w, h)) - QT_PSNR) < 5e-3
    # a carried-in avgError (FC:20, never reset) changes the first iteration's sum exactly as in the model
    assert _same_decode(fic_amd.decode_rgb_quadtree_run(run, avg_error_in=3.25), rm.decode(run, avg_error_in=3.25))


def test_multi_workgroup_compaction_1024():
    lena = np.load(os.path.join(GOLDEN, "lena_colored_256.npy"))
    rgb = np.stack([synth.enlarge(np.ascontiguousarray(lena[..., c]), 1024, 1024) for c in range(3)], axis=-1)
    argb, w, h = fo.rgb_to_argb(rgb), 1024, 1024
    cbs = _gpu_codebooks(argb, w, h, 16, 4, 0)
    sse = capi.debug_rgb_quadtree_sse(argb, w, h, 16, 4, 0)
    inf = fic_amd.encode_rgb_quadtree(argb, w, h, 16, 4, 0, INF)
    assert len(inf) == 4096 and (inf[:, 3:] == cbs[16]).all()
    neg = fic_amd.encode_rgb_quadtree(argb, w, h, 16, 4, 0, -1.0)
    j = neg[:, 1] // 4 * (w // 4) + neg[:, 0] // 4
    assert len(neg) == 65536 and (np.sort(j) == np.arange(65536)).all() and (neg[:, 3:] == cbs[4][j]).all()
    mid = fic_amd.encode_rgb_quadtree(argb, w, h, 16, 4, 0, 60.0)
    want = rm.leaf_table(rm.split(sse, w, h, 16, 4, 60.0), cbs, w)
    assert 4096 < len(mid) < 65536 and mid.shape == want.shape and (mid == want).all()


def test_refusals():
    argb, w, h = _image("U64")
    leaves = fic_amd.encode_rgb_quadtree(argb, w, h, 16, 4, 0, 200.0)
    run = fic_amd.write_run_rgb_quadtree(leaves, w, h, 16, 4, 0)
    # no existing reader accepts a tag-3 stream
    for fn, code in ((fic_amd.decode_gray_run, -6), (fic_amd.decode_rgb_run, -1), (fic_amd.decode_quadtree_run, -3)):
        with pytest.raises(fic_amd.FicError) as e:
            fn(run)
        assert e.value.code == code, fn.__name__
    bad_idx = bytearray(run)
    bad_idx[36:40] = (10 ** 6).to_bytes(4, "big")
    for name, bad in {"tag0": b"\0\0\0\0" + run[4:], "tag1": b"\0\0\0\1" + run[4:], "tag2": b"\0\0\0\2" + run[4:],
                      "truncated": run[:-4], "oversized": run + b"\0\0\0\0", "bad_idx_local": bytes(bad_idx)}.items():
        with pytest.raises(fic_amd.FicError) as e:
            fic_amd.decode_rgb_quadtree_run(bad)
        assert e.value.code == -3, name
    with pytest.raises(fic_amd.FicError) as e:
        fic_amd.encode_rgb_quadtree(argb, w, h, 16, 4, 0, float("nan"))
    assert e.value.code == -3
    # capacity: the count is still reported
    out = np.zeros((len(leaves) - 1, 8), np.int32)
    n = C.c_int(-1)
    rc = capi.lib().fic_encode_rgb_quadtree_argb(capi.ptr(np.ascontiguousarray(argb), C.c_int32), w, h, 16, 4, 0, 200.0, 0,
                                                 capi.ptr(out, C.c_int32), out.shape[0], C.byref(n))
    assert rc == -8 and n.value == len(leaves)
    img = np.zeros((h, w), np.int32)
    rc = capi.lib().fic_decode_rgb_quadtree_run(capi.ptr(np.frombuffer(run, np.uint8), C.c_uint8), len(run), 0,
                                                capi.ptr(img, C.c_int32), w * h - 1, None, None, None, None)
    assert rc == -8
