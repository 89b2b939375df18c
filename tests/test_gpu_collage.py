"""The grey collage kernel k_collage (fic_ctx_collage_host, what FractalCompression.encode returns) end to end, against the
numpy model tests/greyisomodel.py on the ORACLE's codebook: through the winning isometry (n_iso = 8), for every plane of a batch,
on non-square and minimum geometries, after every sweep that can have built the pool, and where the value leaves 0..255 before
the clamp.  idx_global -- the array the kernel reads -- is compared with calculateIndices of the oracle's window-local index.
The painter-agreement inequality (greyisomodel's docstring) is checked on the device's own arrays, so what the encoder and the
painters mean by isometry k is pinned by more than bit parity with the oracle."""
import ctypes as C
import io

import numpy as np
import pytest

import fic_amd
import greyisomodel as gm
from fic_amd import capi, synth
from conftest import same_f32

pytestmark = pytest.mark.gpu
E_ARGUMENT, E_STATE = -3, -7
BLACK = np.int32(-16777216)                                           # 0xFF000000: what a NaN fit paints

_IMAGES = {}
_ORACLE = {}


def _image(name, lena64, lena_grey):
    if name not in _IMAGES:
        _IMAGES[name] = {"lena64": lambda: lena64,
                         "crop": lambda: np.ascontiguousarray(lena_grey[64:192, 64:192]),
                         "overshoot": gm.overshoot_image,
                         "U96x64": lambda: synth.image_u(96, 64, 7),
                         "S64x96": lambda: synth.image_s(64, 96, 9),
                         "S16": lambda: synth.image_s(16, 16, 9),
                         "U32x16": lambda: synth.image_u(32, 16, 7),
                         "flat": lambda: np.full((64, 64), 77, np.uint8)}[name]()
    return _IMAGES[name]


def _oracle_encode(oracle, name, g, B, wK, n_iso):
    """The oracle's codebook, once per case: idx_local, the pool index of calculateIndices, a, b, iso, err."""
    key = (name, B, wK, n_iso)
    if key not in _ORACLE:
        h, w = g.shape
        r = oracle.encode_gray(oracle.gray_to_argb(g), w, h, B, wK, n_iso)
        r["idx_local"] = r["info"][:, 0].astype(np.int32)
        r["idx_global"] = gm.to_global(w, h, B, wK, r["info"][:, 0])
        _ORACLE[key] = r
    return _ORACLE[key]


def _same_codebook(got, ref, plane=0):
    assert (got["idx_local"][plane] == ref["idx_local"]).all()
    assert (got["iso"][plane] == ref["iso"]).all()
    assert same_f32(got["a"][plane], ref["info"][:, 1])
    assert same_f32(got["b"][plane], ref["info"][:, 2])
    assert same_f32(got["err"][plane], ref["err"])
    assert (got["idx_global"][plane] == ref["idx_global"]).all()


# image, B, wK, sweeps (0: automatic; a windowed search has no other), all 8 isometries win somewhere
CASES = [("lena64", 4, 29, (1, 2, 6), True), ("lena64", 8, 13, (1, 2, 5, 6), True), ("crop", 16, 13, (1, 2, 6), True),
         ("overshoot", 4, 29, (1, 2, 6), False), ("overshoot", 4, 5, (0,), False), ("overshoot", 8, 3, (0,), False),
         ("U96x64", 8, 3, (0,), False), ("S64x96", 4, 5, (0,), False), ("S16", 8, 1, (0,), False), ("U32x16", 8, 1, (0,), False)]
IDS = [f"{c[0]}-B{c[1]}-wK{c[2]}" for c in CASES]


def _encoded(enc, sweep, B):
    """One encode of `enc` through `sweep`: (results, collage), with the sweep that ran checked."""
    enc.set_option("sweep", sweep)
    enc.encode()
    if sweep:
        assert enc.info()["sweep_kind"] == sweep
    if sweep == 6 and B != 8:                                         # k_pool_q built this pool, not the fused small launch
        assert "k_prep_q8" not in enc.last_kernel()
    return enc.results(), enc.collage()


@pytest.mark.parametrize("name,B,wK,sweeps,all_k", CASES, ids=IDS)
def test_collage_through_the_winning_isometry(oracle, lena64, lena_grey, name, B, wK, sweeps, all_k):
    g = _image(name, lena64, lena_grey)
    h, w = g.shape
    ref = _oracle_encode(oracle, name, g, B, wK, 8)
    want, v = gm.collage(g, B, ref["idx_global"], ref["info"][:, 1], ref["info"][:, 2], ref["iso"])
    if name == "overshoot":                                           # the clamp has work to do at both ends
        assert (v < 0).any() and (v >= 256).any()
    if all_k:
        assert set(np.unique(ref["iso"])) == set(range(8))
    with fic_amd.Encoder(w, h, B, wK, 8) as enc:
        enc.set_gray(g)
        for sweep in sweeps:
            res, col = _encoded(enc, sweep, B)
            _same_codebook(res, ref)
            assert (col[0] == want).all(), f"sweep {sweep}: {int((col[0] != want).sum())} pixels differ"


@pytest.mark.parametrize("name,B,wK,sweeps,all_k", CASES, ids=IDS)
def test_collage_with_one_isometry_is_the_oracles(oracle, lena64, lena_grey, name, B, wK, sweeps, all_k):
    """The reference algorithm, against fo_collage_gray itself.  (Sweep 5, k_sweep_d4, exists for n_iso = 8 only.)"""
    g = _image(name, lena64, lena_grey)
    h, w = g.shape
    ref = _oracle_encode(oracle, name, g, B, wK, 1)
    want = oracle.collage_gray(oracle.gray_to_argb(g), w, h, B, wK, ref["info"])
    with fic_amd.Encoder(w, h, B, wK, 1) as enc:
        enc.set_gray(g)
        for sweep in sweeps:
            if sweep == 5:
                continue
            res, col = _encoded(enc, sweep, B)
            _same_codebook(res, ref)
            assert (res["iso"] == 0).all()
            assert (col[0] == want).all(), f"sweep {sweep}: {int((col[0] != want).sum())} pixels differ"


@pytest.mark.parametrize("B,wK", [(8, None), (4, 5)])
def test_every_plane_gets_its_own_collage(oracle, lena64, lena_grey, B, wK):
    """Three different images in one context: each plane's collage is the model's on that plane's oracle codebook, and the flat
    plane in the middle (every fit NaN) is black."""
    names = ["lena64", "flat", "overshoot"]
    stack = np.stack([_image(n, lena64, lena_grey) for n in names])
    with fic_amd.Encoder(64, 64, B, wK, 8, planes=3) as enc:
        enc.set_gray(stack)
        enc.encode()
        res, col = enc.results(), enc.collage()
        wk = enc.wK
    for p, name in enumerate(names):
        ref = _oracle_encode(oracle, name, stack[p], B, wk, 8)
        _same_codebook(res, ref, p)
        want, _ = gm.collage(stack[p], B, ref["idx_global"], ref["info"][:, 1], ref["info"][:, 2], ref["iso"])
        assert (col[p] == want).all(), f"plane {p}: {int((col[p] != want).sum())} pixels differ"
    assert (col[1] == BLACK).all()
    assert (col[0] != col[2]).any()


@pytest.mark.parametrize("name,B", [("lena64", 4), ("lena64", 8), ("crop", 16)])
def test_encoder_and_painters_agree_on_the_isometry_ids(lena64, lena_grey, name, B):
    """greyisomodel.painter_agreement on the device's own pool, pool indices, contrasts and isometry ids (full search)."""
    g = _image(name, lena64, lena_grey)
    h, w = g.shape
    with fic_amd.Encoder(w, h, B, None, 8) as enc:
        enc.set_gray(g)
        enc.encode()
        res = enc.results()
        pix = enc.debug_pool()["pix"][0]
    gm.check_agreement(gm.painter_agreement(g, B, pix, res["idx_global"][0], res["a"][0], res["iso"][0]))


def test_mirror_returns_the_collage_of_the_eight_isometry_search(oracle, lena64):
    fc = fic_amd.FractalCompression
    ref = _oracle_encode(oracle, "lena64", lena64, 4, 29, 8)
    want, _ = gm.collage(lena64, 4, ref["idx_global"], ref["info"][:, 1], ref["info"][:, 2], ref["iso"])
    img = fic_amd.RasterImage.from_gray(lena64)
    try:
        fc.n_iso, fc.blockgroesse, fc.widthKernel = 8, 4, 29
        collage = fc.encode(img, io.BytesIO())
        assert (collage.argb == want).all()
        assert (fc.getBestGeneratedCollage(img).argb == want).all()
        assert (fc.imageIso == ref["iso"]).all() and (fc.imageIso != 0).any()
    finally:
        fc.n_iso, fc.blockgroesse, fc.widthKernel, fc.avgError = 1, 8, 2, np.float32(0.0)


def test_collage_needs_an_encode_and_an_output(lena64):
    with fic_amd.Encoder(64, 64, 8, 13, 8) as enc:
        enc.set_gray(lena64)
        with pytest.raises(fic_amd.FicError) as e:
            enc.collage()
        assert e.value.code == E_STATE
        enc.encode()
        with pytest.raises(fic_amd.FicError) as e:
            capi.check(capi.lib().fic_ctx_collage_host(enc._h, C.POINTER(C.c_int32)()))
        assert e.value.code == E_ARGUMENT
        assert enc.collage().shape == (1, 64 * 64)
