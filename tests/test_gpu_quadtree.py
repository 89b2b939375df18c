"""Quadtree (variable block size) grey codec on the GPU against the numpy model (tests/qtmodel.py): per-level collage SSE, the
leaf table for several thresholds, and the decoder (pixels, avgError bits, iterations).  The model runs on the GPU's own
fixed-level one-shot codebooks, which the quadtree encode must reproduce level by level.  DESIGN.md section 4.13."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qtmodel as qm  # noqa: E402

import fic_amd  # noqa: E402
from fic_amd import capi, synth  # noqa: E402
from oracle import fic_oracle as fo  # noqa: E402

pytestmark = pytest.mark.gpu

INF = float("inf")
THRESHOLDS = (INF, 400.0, 60.0, 0.0, -1.0)


def _image(name):
    if name == "lena256":
        return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lena_grey_256.npy"))
    kind, n = name[0], int(name[1:])
    return synth.image(kind, n, n, synth.SEEDS["cfg2"] + n)


def _gpu_codebooks(g, B_max, B_min, wK, n_iso):
    h, w = g.shape
    out = {}
    for B in qm.levels(B_max, B_min):
        r = capi.encode_gray_oneshot(g, B, qm.level_wk(w, h, B, wK), n_iso)
        out[B] = (r["qrows"], r["iso"] if n_iso == 8 else np.zeros_like(r["iso"]))
    return out


def _same_decode(a, b):
    return bool((a[0] == b[0]).all() and a[1].view(np.uint32) == b[1].view(np.uint32) and a[2] == b[2])


CASES = [
    ("U64", 16, 4, 0, 1), ("S64", 16, 4, 2, 8), ("U128", 8, 4, 2, 1), ("S128", 16, 8, 0, 8),
    ("lena256", 16, 4, 0, 1), ("lena256", 16, 4, 2, 8),
]


@pytest.mark.parametrize("name,B_max,B_min,wK,n_iso", CASES)
def test_quadtree_matches_model(name, B_max, B_min, wK, n_iso):
    g = _image(name)
    h, w = g.shape
    cbs = _gpu_codebooks(g, B_max, B_min, wK, n_iso)
    sse = qm.level_sse(g, cbs, wK)
    got = capi.debug_quadtree_sse(g, B_max, B_min, wK, n_iso)
    for B in qm.levels(B_max, B_min):
        assert (got[B].astype(np.int64) == sse[B]).all(), f"SSE at B={B}"
    for t in THRESHOLDS:
        leaves = fic_amd.encode_gray_quadtree(g, B_max, B_min, wK, n_iso, t)
        want = qm.leaf_table(qm.split(sse, w, h, B_max, B_min, t), cbs, w)
        assert leaves.shape == want.shape and (leaves == want).all(), f"leaf table at threshold {t}"
        if t == INF:          # the fixed-B_max rows in scanline order
            q, k = cbs[B_max]
            assert (leaves[:, 3:6] == q).all() and (leaves[:, 6] == k).all()
        if t < 0:             # every B_min row, depth first
            assert (leaves[:, 2] == B_min).all() and len(leaves) == (w // B_min) * (h // B_min)
        if t in (INF, 60.0, -1.0):
            run = fic_amd.write_run_quadtree(leaves, w, h, B_max, B_min, wK, n_iso)
            assert run == qm.write_run(want, w, h, B_max, B_min, wK, n_iso)
            dec = fic_amd.decode_quadtree_run(run)
            assert _same_decode(dec, qm.decode(run)), f"decode at threshold {t}"
            if t == INF and n_iso == 1:
                fixed = fic_amd.write_run_gray(cbs[B_max][0], w, h, B_max, qm.level_wk(w, h, B_max, wK))
                assert _same_decode(dec, fic_amd.decode_gray_run(fixed))


def test_argb_twin_and_avg_error_carry():
    g = _image("lena256")
    h, w = g.shape
    a = fic_amd.encode_gray_quadtree(g, 16, 4, 0, 1, 400.0)
    b = fic_amd.encode_gray_quadtree(fo.gray_to_argb(g).reshape(h, w), 16, 4, 0, 1, 400.0)
    assert (a == b).all()
    assert len(a) == 937           # the CPU calibration (test_quadtree_model.QT_LEAVES)
    run = fic_amd.write_run_quadtree(a, w, h, 16, 4, 0, 1)
    img, avg, it = fic_amd.decode_quadtree_run(run)
    assert abs(fo.psnr(img, g) - 24.872) < 5e-3
    # a carried-in avgError (FC:20, never reset) changes the first iteration's sum exactly as in the model
    assert _same_decode(fic_amd.decode_quadtree_run(run, avg_error_in=3.25), qm.decode(run, avg_error_in=3.25))


def test_multi_workgroup_compaction_1024():
    g = synth.enlarge(_image("lena256"), 1024, 1024)
    h, w = g.shape
    cbs = _gpu_codebooks(g, 16, 4, 0, 1)
    sse = capi.debug_quadtree_sse(g, 16, 4, 0, 1)
    inf = fic_amd.encode_gray_quadtree(g, 16, 4, 0, 1, INF)
    assert len(inf) == 4096 and (inf[:, 3:6] == cbs[16][0]).all()
    neg = fic_amd.encode_gray_quadtree(g, 16, 4, 0, 1, -1.0)
    j = neg[:, 1] // 4 * (w // 4) + neg[:, 0] // 4
    assert len(neg) == 65536 and (np.sort(j) == np.arange(65536)).all() and (neg[:, 3:6] == cbs[4][0][j]).all()
    mid = fic_amd.encode_gray_quadtree(g, 16, 4, 0, 1, 20.0)
    want = qm.leaf_table(qm.split(sse, w, h, 16, 4, 20.0), cbs, w)
    assert 4096 < len(mid) < 65536 and mid.shape == want.shape and (mid == want).all()
