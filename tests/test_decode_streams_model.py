"""CPU checks of the hand-built decoder inputs of tests/streammodel.py, on the reference models alone:
they prove what tests/test_gpu_decode_streams.py claims to cover -- every (side, isometry) pair and that the isometry shows
in the decoded pixels at every zoom, the pool's corners, the clamp on both sides, Java's float-to-int saturation, 50
iterations on all four tags -- so the GPU tests cannot pass vacuously.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qtmodel as qm  # noqa: E402
import qtrgbmodel as rm  # noqa: E402
import rgbisomodel as rim  # noqa: E402
import streammodel as sm  # noqa: E402
import zoommodel as zm  # noqa: E402

from oracle import fic_oracle as fo  # noqa: E402

ZOOMS = (1, 2, 4)
QT_CASES, FIXED_CASES = sm.QT_CASES, sm.FIXED_CASES


def _same(a, b):
    return bool(a[0].shape == b[0].shape and (a[0] == b[0]).all() and np.float32(a[1]).view(np.uint32) == np.float32(b[1]).view(np.uint32)
                and a[2] == b[2])


def _leaf(img, leaf, z):
    x, y, B = (int(v) * z for v in leaf[:3])
    return img[y:y + B, x:x + B]


@pytest.mark.parametrize("w,h,wK,seed", QT_CASES)
def test_quadtree_cases_parse_and_cover(oracle, w, h, wK, seed):
    g, c = sm.grey_quadtree_case(w, h, wK, seed), sm.rgb_quadtree_case(w, h, wK, seed)
    hd, leaves = qm.read_run(g["run"])
    assert hd == dict(w=w, h=h, B_max=16, B_min=4, wK=wK, n_iso=8) and (leaves == g["leaves"]).all()
    chd, cleaves = rm.read_run(c["run"])
    assert chd == dict(w=w, h=h, B_max=16, B_min=4, wK=wK) and (cleaves == c["leaves"]).all()
    assert (cleaves[:, :3] == leaves[:, :3]).all()                                    # the same tree
    assert {(int(b), int(k)) for b, k in leaves[:, [2, 6]]} == {(b, k) for b in (4, 8, 16) for k in range(8)}
    # the tree: >= 8 top blocks stay leaves, >= 2 are four 8-leaves, >= 2 hold 8-leaves and 4-leaves; depths interleaved
    kinds = {}
    for x, y, b in leaves[:, :3]:
        kinds.setdefault((x // 16, y // 16), set()).add(int(b))
    count = lambda s: sum(1 for v in kinds.values() if v == s)  # noqa: E731
    assert count({16}) >= 8 and count({8}) >= 2 and count({8, 4}) >= 2
    sides = leaves[:, 2]
    assert (sides[1:] != sides[:-1]).sum() >= 8                                      # interleaved in stream order, not grouped
    # the pool's corners, per level
    for case in (g, c):
        for B in (16, 8, 4):
            got = set(sm.resolved_indices(case, B).tolist())
            want = [t for _, _, t in sm.corner_targets(w, h, B, wK)]
            assert set(want) <= got, (B, want)
            Rw, Rh, Dw, Dh = fo.geometry(w, h, B)
            if wK == 0 or wK >= 5:
                assert want == sm.pool_corners(w, h, B)
            else:                                                                   # no window of any range block reaches farther
                G = sm.window_table(w, h, B, wK)
                assert want[0] == 0 and want[3] == G.max() and want[3] % Dw == (G % Dw).max() and want[3] // Dw == (G // Dw).max()
    # every designated row is there, per side
    assert set(g["designated"]) == {(b, n) for b in (4, 8, 16) for n in sm.GREY_ROWS}
    assert set(c["designated"]) == {(b, n) for b in (4, 8, 16) for n in sm.RGB_ROWS}
    for (b, n), i in g["designated"].items():
        assert leaves[i, 2] == b and tuple(leaves[i, 4:6]) == sm.GREY_ROWS[n]
    for (b, n), i in c["designated"].items():
        assert cleaves[i, 2] == b and tuple(cleaves[i, 4:8]) == sm.RGB_ROWS[n]


def test_domain_blocks_are_not_symmetric_after_the_first_iteration(oracle):
    """After one paint from the flat start every leaf is a constant; the 32 x 32 domain region of a side-16 leaf spans leaves
    with different rows and is then no longer symmetric: per isometry k != 0 some side-16 leaf's domain block differs from its
    image under k, so from iteration 2 on a wrong isometry changes pixels.  (The domain regions of the smaller sides often lie
    inside one leaf and take their texture an iteration or two later: test_every_isometry_shows_at_every_side_and_zoom.)"""
    for w, h, wK, seed in QT_CASES:
        case = sm.grey_quadtree_case(w, h, wK, seed)
        lv = case["leaves"]
        img = np.full((h, w), 128, np.uint8)
        for x, y, B, _, qa, qb, _ in lv:
            v = qm.paint_values(np.full((h, w), 128, np.uint8), B, np.array([0]), [qa], [qb], [0])[0, 0]
            img[y:y + B, x:x + B] = v
        for B in (16,):
            pix = fo.pool(fo.gray_to_argb(img), w, h, B)[0][sm.resolved_indices(case, B)]
            T = qm.iso_table(B)
            ks = lv[lv[:, 2] == B][:, 6]
            moved = {int(k) for p, k in zip(pix, ks) if k and (p[T[k]] != p).any()}   # the leaf's own isometry moves its block
            assert moved == set(range(1, 8)), (w, h, wK, B)


@pytest.mark.parametrize("w,h,wK,seed", QT_CASES)
def test_every_isometry_shows_at_every_side_and_zoom(oracle, w, h, wK, seed):
    """Zero insensitive pairs: for every zoom z and every (z * side, k != 0) at least one leaf of that side and isometry holds
    a pixel that changes when the stream's isometry column is zeroed."""
    case = sm.grey_quadtree_case(w, h, wK, seed)
    lv = case["leaves"].copy()
    lv[:, 6] = 0
    plain = qm.write_run(lv, w, h, 16, 4, wK, 8)
    for z in ZOOMS:
        a, b = sm.reference(case["run"], z)[0], zm.decode_quadtree(plain, z)[0]
        seen = {(z * int(l[2]), int(l[6])) for l in case["leaves"] if l[6] and (_leaf(a, l, z) != _leaf(b, l, z)).any()}
        want = {(z * s, k) for s in (4, 8, 16) for k in range(1, 8)}
        assert seen == want, (z, sorted(want - seen))


def _lut(a, b):
    """clamp((int) fl(fl(a * d) + b)) for d = 0..255 through the oracle's own fo_java_f2i."""
    L = fo.lib()
    d = np.arange(256, dtype=np.float32)
    v = (np.float32(a) * d).astype(np.float32) + np.float32(b)
    return np.array([min(255, max(0, L.fo_java_f2i(float(x)))) for x in v.astype(np.float32)], np.int64)


def test_saturation_rows_against_java_f2i(oracle):
    """The (int) cast saturates (JLS 5.1.3) before the clamp: the numpy models' trunc + clip agree with fo_java_f2i on the
    designated rows for every domain pixel value, and the saturation rows give 0 or 255 only, on the side Java gives."""
    d = np.arange(256, dtype=np.uint8)
    scaled = np.stack([np.tile(np.arange(260) % 256, (4, 1))] * 3, axis=-1)       # a colour pool of 257 x 1 blocks of side 4
    gi = np.arange(253)
    for name, (qa, qb) in sm.GREY_ROWS.items():
        lut = _lut(np.float32(qa) / np.float32(100), np.float32(qb))
        v = np.clip(np.trunc((np.float32(qa) / np.float32(100) * d.astype(np.float32)).astype(np.float32) + np.float32(qb)).astype(np.int64), 0, 255)
        assert (v == lut).all(), name
        if name in sm.GREY_CONSTANT:
            assert (lut == sm.GREY_CONSTANT[name]).all(), name
    up, down, top = _lut(np.float32(sm.INT_MAX) / np.float32(100), np.float32(sm.INT_MIN)), \
        _lut(np.float32(sm.INT_MIN) / np.float32(100), np.float32(sm.INT_MAX)), _lut(np.float32(sm.INT_MAX) / np.float32(100), np.float32(sm.INT_MAX))
    assert set(up) == set(down) == {0, 255} and (top == 255).all()
    assert (up[:101] == 0).all() and (up[101:] == 255).all() and (down[:100] == 255).all() and (down[100:] == 0).all()
    for name, q in sm.RGB_ROWS.items():
        a = np.float32(q[0]) / np.float32(1e6)
        bs = (np.float32(q[1]) / np.float32(1e5), np.float32(q[2]) / np.float32(1e5), np.float32(q[3]))
        got = rm.paint_values(scaled, 4, gi, [(0,) + tuple(q)] * gi.size)           # [253, 16, 3]: pixel = gi + position % 4
        for c in range(3):
            lut = _lut(a, bs[c])
            assert (got[:, :, c] == lut[gi[:, None] + np.arange(16)[None, :] % 4]).all(), (name, c)
        if name in sm.RGB_CONSTANT:
            assert (got == np.array(sm.RGB_CONSTANT[name])).all(), name
        else:
            assert set(got[:, :, 2].reshape(-1)) <= {0, 255}, name                 # bB = +-2^31: the channel that saturates


@pytest.mark.parametrize("w,h,wK,seed", QT_CASES)
def test_clamp_leaves_in_the_reference_decode(oracle, w, h, wK, seed):
    g, c = sm.grey_quadtree_case(w, h, wK, seed), sm.rgb_quadtree_case(w, h, wK, seed)
    for z in (1, 4):
        img = sm.reference(g["run"], z)[0]
        for (B, name), i in g["designated"].items():
            px = _leaf(img, g["leaves"][i], z)
            if name in sm.GREY_CONSTANT:
                assert (px == sm.GREY_CONSTANT[name]).all(), (z, B, name)
            elif name in ("max_min", "min_max"):
                assert set(px.reshape(-1)) <= {0, 255}, (z, B, name)
        rgb = sm.reference(c["run"], z)[0]
        for (B, name), i in c["designated"].items():
            px = _leaf(rgb, c["leaves"][i], z)
            if name in sm.RGB_CONSTANT:
                assert (px == np.array(sm.RGB_CONSTANT[name])).all(), (z, B, name)
            elif name == "max_max":
                assert (px[..., 2] == 255).all(), (z, B)
            else:
                assert set(px[..., 2].reshape(-1)) <= {0, 255}, (z, B, name)
    # both sides of the clamp are reached by ordinary rows as well: pixels at 0 and at 255 next to values strictly inside
    img = sm.reference(g["run"], 1)[0]
    assert (img == 0).any() and (img == 255).any() and ((img > 0) & (img < 255)).any()


@pytest.mark.parametrize("tag,w,h,B,wK,seed", FIXED_CASES)
def test_fixed_cases(oracle, tag, w, h, B, wK, seed):
    case = sm.fixed_case(tag, w, h, B, wK, seed)
    Rw, Rh, Dw, Dh = fo.geometry(w, h, B)
    rows = case["rows"]
    gi = qm.global_index(w, h, B, case["wK"], rows[:, 0])
    want = [t for _, _, t in sm.corner_targets(w, h, B, wK)]
    assert set(want) <= set(gi.tolist())
    if wK == 0:
        assert want == sm.pool_corners(w, h, B)
    assert set(case["designated"]) == set(sm.RGB_ROWS if tag else sm.GREY_ROWS)
    img, avg, it = sm.reference(case["run"], 1)
    assert img.shape[:2] == (h, w) and 1 <= it <= 50
    const = sm.RGB_CONSTANT if tag else sm.GREY_CONSTANT
    for z in (1, 4):
        img = sm.reference(case["run"], z)[0]
        for name, j in case["designated"].items():
            if name in const:
                bx, by = j % Rw, j // Rw
                px = img[z * B * by:z * B * (by + 1), z * B * bx:z * B * (bx + 1)]
                assert (px == np.array(const[name])).all(), (z, name)


def test_zoom_1_is_the_unzoomed_model(oracle):
    for w, h, wK, seed in QT_CASES:
        for run, fn in ((sm.grey_quadtree_case(w, h, wK, seed)["run"], qm.decode), (sm.rgb_quadtree_case(w, h, wK, seed)["run"], rm.decode)):
            for r in (run, sm.oscillating(run)):
                assert _same(sm.reference(r, 1), fn(r)), (w, h, wK)


@pytest.mark.parametrize("name", ["tag0", "tag1", "tag2", "tag3", "tag2_non_square"])
def test_oscillators_run_50_iterations(oracle, name):
    run = sm.oscillators()[name]
    (qm.read_run if run[3] == 2 else rm.read_run if run[3] == 3 else (lambda r: None))(run)
    for z in (1, 4):
        img, avg, it = sm.reference(run, z)
        assert it == 50 and avg >= 1, (name, z, avg)
        if z == 4:
            assert float(avg) * img.shape[0] * img.shape[1] >= 2 ** 24   # the float sum leaves the exact integers (FC:407)


@pytest.mark.parametrize("B,size", [(4, 64), (8, 128), (16, 128)])
def test_tile_image_makes_the_encoder_choose_every_isometry(oracle, B, size):
    img = sm.iso_tile_image(B, size)
    r = fo.encode_gray(fo.gray_to_argb(img), size, size, B, fo.geometry(size, size, B)[2], 8)
    assert set(r["iso"].tolist()) == set(range(8))
    if B in (4, 16):
        rgb = sm.iso_tile_image_rgb(B, size)
        r = rim.encode(fo.rgb_to_argb(rgb), size, size, B, fo.geometry(size, size, B)[2], 8)
        assert set(r["iso"].tolist()) == set(range(8))
