"""The conditions the GPU geometry tests (test_gpu_rgb_geometry.py, test_gpu_quadtree_geometry.py) rest on, checked with the CPU
references alone: every generated case is a geometry and a window the library takes; the fuzz list of the default seed covers
every block size, Rw / Rh = 2, both orientations, full search with 1 and 8 isometries, every image kind and batches; the
8-isometry model equals the oracle's encodeRGB where the oracle is the authority (n_iso = 1) on every minimum geometry and
really uses its isometries on noise; every quadtree level above B_min has a boundary block whose SSE s and threshold
t = float32(s / B^2) meet the split rule `(double) s > (double) t * B * B` at equality, so that t and its float32 predecessor
give different leaves; the S planes hold blocks of SSE 0, which +0.0 and -0.0 both leave whole."""
import numpy as np
import pytest

import geomcases as gc
import qtmodel as qm
import rgbisomodel as rim
from conftest import same_f32
from fic_amd import capi
from oracle import fic_oracle as fo

E_GEOMETRY, E_WINDOW = -1, -2


@pytest.mark.parametrize("c", gc.RGB_CASES, ids=gc.case_id)
def test_fixed_case_is_accepted(c):
    """fic_geometry takes the image, and the host-side window check (the tag-5 writer runs the encoders' make_geometry) takes wK."""
    Rw, Rh, Dw, Dh = capi.geometry(c.w, c.h, c.B)
    assert (Rw, Rh, Dw, Dh) == gc.dims(c) == fo.geometry(c.w, c.h, c.B)
    assert 1 <= c.wK <= min(Dw, Dh) and c.n_iso in (1, 8) and 1 <= c.planes <= 3 and c.kind in gc.KINDS
    run = capi.write_run_rgb_iso(np.zeros((Rw * Rh, 5), np.int32), np.zeros(Rw * Rh, np.int32), c.w, c.h, c.B, c.wK)
    assert len(run) == 24 + 24 * Rw * Rh
    for bad in (0, min(Dw, Dh) + 1):                     # the check is live: the neighbours of the valid windows are refused
        with pytest.raises(capi.FicError) as e:
            capi.write_run_rgb_iso(np.zeros((Rw * Rh, 5), np.int32), np.zeros(Rw * Rh, np.int32), c.w, c.h, c.B, bad)
        assert e.value.code == E_WINDOW
    imgs = gc.case_images(c, 0)
    assert imgs.shape == (c.planes, c.w * c.h)
    if c.kind != "lena":                                 # a Lena crop may repeat; every other kind gives another image per plane
        assert len({imgs[p].tobytes() for p in range(c.planes)} | {gc.case_images(c, 1)[-1].tobytes()}) == c.planes + 1


@pytest.mark.parametrize("c", gc.QT_CASES, ids=gc.qt_case_id)
def test_quadtree_case_is_accepted(c):
    """Every level of the tree is a geometry with the case's window (wK = 0: the level's whole pool, square images only), and
    the quadtree writer, which runs the encoders' level check, takes the header."""
    assert c.B_max in (8, 16) and c.B_min in (4, 8) and c.B_min < c.B_max and c.w % c.B_max == 0 and c.h % c.B_max == 0
    assert c.wK > 0 or c.w == c.h
    for B in qm.levels(c.B_max, c.B_min):
        Rw, Rh, Dw, Dh = capi.geometry(c.w, c.h, B)
        assert 1 <= qm.level_wk(c.w, c.h, B, c.wK) <= min(Dw, Dh)
    n = (c.w // c.B_max) * (c.h // c.B_max)
    leaves = np.zeros((n, 9), np.int32)
    j = np.arange(n)
    leaves[:, 0], leaves[:, 1], leaves[:, 2] = j % (c.w // c.B_max) * c.B_max, j // (c.w // c.B_max) * c.B_max, c.B_max
    assert len(capi.write_run_rgb_quadtree_iso(leaves, c.w, c.h, c.B_max, c.B_min, c.wK)) == 32 + 28 * n


def test_tables_and_ids():
    assert len(gc.MIN_CASES) == 28 and len(gc.QT_CASES) == 18
    assert {(c.w, c.h, c.B, c.wK) for c in gc.MIN_CASES} == set(gc.MIN_GEOMETRIES)
    ids = [gc.case_id(c) for c in gc.RGB_CASES] + [gc.qt_case_id(c) for c in gc.QT_CASES]
    assert len(set(ids)) == len(ids)
    assert gc._fuzz(gc.FUZZ_SEED, 5) == gc._fuzz(gc.FUZZ_SEED, 5) == gc.FUZZ_CASES[:5]          # deterministic, a prefix of itself
    for c in gc.FUZZ_CASES:
        Rw, Rh, Dw, Dh = gc.dims(c)
        assert 2 <= Rw <= min(24, 160 // c.B) and 2 <= Rh <= min(24, 160 // c.B)
        assert not (gc.is_full(c) and c.n_iso == 8) or c.w <= 96      # bounds the numpy model's time


def test_fuzz_list_covers_what_the_gpu_tests_claim():
    F = gc.FUZZ_CASES
    assert {c.B for c in F} == {4, 8, 16}
    assert any(c.w // c.B == 2 for c in F) and any(c.h // c.B == 2 for c in F)
    assert any(c.w > c.h for c in F) and any(c.h > c.w for c in F)
    for n_iso in (1, 8):
        assert any(gc.is_full(c) and c.n_iso == n_iso for c in F), n_iso
        assert any(not gc.is_full(c) and c.n_iso == n_iso for c in F), n_iso
        assert any(c.w > c.h and c.n_iso == n_iso for c in F), n_iso                 # the x + 1 >= HEIGHT quirk of scaleImageRGB
    assert {c.kind for c in F} == set(gc.KINDS)
    assert {c.planes for c in F} == {1, 2, 3}
    assert any(gc.is_full(c) and c.n_iso == 8 and c.B == 16 for c in F)             # always the matrix-core mode
    assert any(gc.is_full(c) and c.n_iso == 8 and c.kind in ("const", "low") for c in F)     # isometry ties inside a candidate
    for kind in ("const", "low"):
        assert any(not gc.is_full(c) and c.n_iso == 8 and c.kind == kind for c in F), kind


@pytest.mark.parametrize("c", [c for c in gc.MIN_CASES if c.n_iso == 1], ids=gc.case_id)
def test_model_equals_the_oracle_with_one_isometry(c):
    """rgbisomodel.encode(n_iso = 1) is fo_encode_rgb bit for bit (NaNs counted equal), collage and decode included."""
    for p in range(c.planes):
        argb = gc.argb_image(c.kind, c.w, c.h, c.seed, p)
        ref = gc.case_reference(c, p)
        got = rim.encode(argb, c.w, c.h, c.B, c.wK, 1)
        assert same_f32(got["info"], ref["info"]) and (got["iso"] == 0).all() and (got["qrows"] == ref["qrows"]).all()
        assert (rim.collage(argb, c.w, c.h, c.B, c.wK, got["info"], got["iso"]) == ref["collage"]).all()
        img, avg, it = rim.decode(got["qrows"], got["iso"], c.w, c.h, c.B, c.wK)
        assert (img == ref["decode"][0]).all() and same_f32(avg, ref["decode"][1]) and it == ref["decode"][2]


@pytest.mark.parametrize("w,h", [(48, 48), (64, 32)])
def test_eight_isometry_model_uses_its_isometries_on_noise(w, h):
    c = next(c for c in gc.MIN_CASES if (c.w, c.h, c.n_iso) == (w, h, 8))
    assert c.kind == "noise"
    assert len(np.unique(gc.case_reference(c, 0)["iso"])) >= 4


def _leaf(tree, x, y, B):
    return (x, y, B) in set(tree)


@pytest.mark.parametrize("encoder", gc.QT_ENCODERS)
@pytest.mark.parametrize("c", gc.QT_CASES, ids=gc.qt_case_id)
def test_split_rule_at_equality(c, encoder):
    """Every level above B_min has a boundary block, in both image kinds: float(t) * B * B == s exactly, the block is a leaf
    at t and split at the float32 just below."""
    sse = gc.qt_reference(c, encoder)["sse"]
    for B in qm.levels(c.B_max, c.B_min)[:-1]:
        b = gc.qt_boundary(c, sse, B)
        assert b is not None, f"no boundary block at B={B}"
        x, y, s, t = b
        assert t.dtype == np.float32 and 0 < s < 1 << 24 and int(sse[B][y // B, x // B]) == s
        assert float(t) * B * B == s                                          # exact in double and in float
        assert float(np.float32(np.float32(t) * np.float32(B * B))) == s
        lo = np.nextafter(t, np.float32(-np.inf))
        at, below = qm.split(sse, c.w, c.h, c.B_max, c.B_min, t), qm.split(sse, c.w, c.h, c.B_max, c.B_min, lo)
        assert at != below and _leaf(at, x, y, B) and not _leaf(below, x, y, B)
        assert len(below) > len(at)


@pytest.mark.parametrize("encoder", gc.QT_ENCODERS)
@pytest.mark.parametrize("c", [c for c in gc.QT_CASES if c.kind == "S"], ids=gc.qt_case_id)
def test_zero_sse_blocks_stay_whole_at_both_zeros(c, encoder):
    sse = gc.qt_reference(c, encoder)["sse"]
    zero = [(int(x) * B, int(y) * B, B) for B in qm.levels(c.B_max, c.B_min)[:-1] for y, x in zip(*np.nonzero(sse[B] == 0))]
    assert zero, "the S planes hold no block of SSE 0 above B_min"
    plus, minus = qm.split(sse, c.w, c.h, c.B_max, c.B_min, 0.0), qm.split(sse, c.w, c.h, c.B_max, c.B_min, -0.0)
    assert plus == minus
    assert any(_leaf(plus, *z) for z in zero)                                 # one the walk reaches: 0 > 0 is false
    assert any(B > c.B_min for _, _, B in plus) and any(B == c.B_min for _, _, B in plus)
    assert plus != qm.split(sse, c.w, c.h, c.B_max, c.B_min, -1.0)            # which splits everything
