"""Least-squares domain search on the GPU (option "search" = 1: k_sweep_lsq_generic / k_sweep_lsq_fast)
against the numpy int64 model tests/lsqmodel.py, bit for bit: idx_local, iso, qrows, E and the bits of a, b, err -- on minimum,
non-square, windowed and ragged geometries, through both sweeps and several pool chunk counts, on inputs that tie everywhere,
clamp qa, and drive qb negative; range spans and batched planes; the cached contexts' hygiene; the streams, the decoders and the
collage on such a codebook; the quadtree with least-squares levels."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import greyisomodel as gm  # noqa: E402
import lsqmodel as lm  # noqa: E402
import qtmodel as qm  # noqa: E402

import fic_amd  # noqa: E402
from fic_amd import capi, synth  # noqa: E402
from conftest import same_f32  # noqa: E402
from oracle import fic_oracle as fo  # noqa: E402

pytestmark = pytest.mark.gpu
E_ARGUMENT, E_STATE = -3, -7
INF = float("inf")

# (w, h, B, wK, chunk counts of the fast sweep besides the automatic one)
GEOMS = [(8, 8, 4, 1, ()), (16, 16, 4, 5, ()), (32, 32, 8, 5, ()), (64, 32, 16, 1, ()), (48, 48, 16, 3, ()),
         (64, 64, 4, 29, (1, 3, 5)), (144, 144, 8, 33, (2,))]
IDS = [f"{g[0]}x{g[1]}-B{g[2]}-wK{g[3]}" for g in GEOMS]
FIELDS = ("idx_local", "idx_global", "iso", "qrows", "E")


def clamp_image(w, h, seed=3):
    """Every 2 x 2 cell is [[255, 0], [0, 255 - e]], e in 0, 4 .. 40: range blocks of full contrast, while the scaled image --
    the cell means 117 .. 127 -- gives domain blocks of almost none, so 100 C / V lies far outside -100 .. 100."""
    e = 4 * np.random.RandomState(seed).randint(0, 11, size=(h // 2, w // 2))
    g = np.zeros((h, w), np.int64)
    g[0::2, 0::2] = 255
    g[1::2, 1::2] = 255 - e
    return g.astype(np.uint8)


def images(w, h):
    y, x = np.mgrid[0:h, 0:w]
    return {"constant": np.full((h, w), 77, np.uint8),
            "checkerboard": np.where(((x >> 1) ^ (y >> 1)) & 1, 200, 40).astype(np.uint8),
            "ramp": (x * 255 // max(w - 1, 1)).astype(np.uint8),
            "U": synth.image_u(w, h, synth.SEEDS["cfg2"] + w),
            "S": synth.image_s(w, h, synth.SEEDS["cfg3"] + h),
            "clamp": clamp_image(w, h)}


_MODEL = {}


def model(name, g, B, wK, n_iso):
    key = (name, g.shape, B, wK, n_iso)
    if key not in _MODEL:
        _MODEL[key] = lm.encode(g, B, wK, n_iso)
    return _MODEL[key]


def assert_same(got, want, what):
    for f in FIELDS:
        assert (np.asarray(got[f]) == want[f]).all(), f"{what}: {f}"
    for f in ("a", "b", "err"):
        assert same_f32(got[f], want[f]), f"{what}: bits of {f}"


def results(enc, plane=0):
    r = {k: v[plane] for k, v in enc.results().items()}
    r["E"] = enc.lsq_error()[plane]
    return r


@pytest.mark.parametrize("n_iso", [1, 8])
@pytest.mark.parametrize("w,h,B,wK,chunks", GEOMS, ids=IDS)
def test_codebook_is_the_models(w, h, B, wK, chunks, n_iso):
    Rw, Rh, Dw, Dh = fo.geometry(w, h, B)
    full = wK == Dw == Dh
    runs = [(1, 0), (0, 0)] + ([(2, 0)] + [(2, c) for c in chunks] if full else [])
    with fic_amd.Encoder(w, h, B, wK, n_iso) as enc:
        enc.set_option("search", "lsq")
        for name, g in images(w, h).items():
            want = model(name, g, B, wK, n_iso)
            enc.set_gray(g)
            got = {}
            for sweep, c in runs:
                enc.set_option("sweep", sweep)
                enc.set_option("chunks", c)
                enc.encode()
                kernel = "k_sweep_lsq_fast" if sweep == 2 or (sweep == 0 and full) else "k_sweep_lsq_generic"
                assert enc.last_kernel() == kernel
                if c:
                    assert enc.info()["chunks"] == c
                got[(sweep, c)] = results(enc)
                assert_same(got[(sweep, c)], want, f"{name}, sweep {sweep}, chunks {c}")
            for key in runs[1:]:                              # the two kernels agree with each other as well
                assert_same(got[key], got[runs[0]], f"{name}, {key} against the generic sweep")
            qa = want["qrows"][:, 1]
            if name == "constant":                            # every pair ties and V = 0: the first candidate wins
                assert (want["idx_local"] == 0).all() and (want["iso"] == 0).all() and (qa == 0).all()
            if name == "clamp" and full and Dw * Dh > 1:
                assert (np.abs(qa) == 100).mean() >= 0.5


def test_three_planes_in_two_spans():
    for B, n_iso in ((4, 8), (8, 1)):
        w = h = 64
        imgs = [images(w, h)[k] for k in ("U", "S", "clamp")]
        want = [model(k, g, B, None, n_iso) for k, g in zip(("U", "S", "clamp"), imgs)]
        with fic_amd.Encoder(w, h, B, None, n_iso, planes=3) as enc:
            enc.set_option("search", "lsq")
            enc.set_gray(np.stack(imgs))
            nr = enc.n_ranges
            cut = nr // 2 + 5                                  # inside a lane tile
            for spans in (((0, -1),), ((0, cut), (cut, nr - cut)), ((cut, -1), (0, cut))):
                for b, c in spans:
                    enc.encode(b, c)
                for p in range(3):
                    assert_same(results(enc, p), want[p], f"B={B}, plane {p}, spans {spans}")


def test_cached_contexts_stay_in_reference_mode(lena64):
    for B, wK, n_iso in ((4, None, 1), (8, 3, 8)):
        before = capi.encode_gray_oneshot(lena64, B, wK, n_iso)
        lsq = capi.encode_gray_oneshot(lena64, B, wK, n_iso, search="lsq")
        after = capi.encode_gray_oneshot(lena64, B, wK, n_iso)
        for k in ("idx_local", "iso", "qrows"):
            assert (before[k] == after[k]).all()
        assert same_f32(before["a"], after["a"]) and same_f32(before["b"], after["b"])
        want = model("lena64", lena64, B, wK, n_iso)
        for k in ("idx_local", "iso", "qrows", "E"):
            assert (lsq[k] == want[k]).all()
        assert same_f32(lsq["a"], want["a"]) and same_f32(lsq["b"], want["b"])
        assert not (lsq["qrows"] == before["qrows"]).all()
        twin = capi.encode_gray_oneshot(fo.gray_to_argb(lena64).reshape(lena64.shape), B, wK, n_iso, search="lsq")
        assert all((twin[k] == lsq[k]).all() for k in ("idx_local", "iso", "qrows", "E"))
        # the handle API gives the same rows (the context of fic_amd.encode_gray is its own)
        r = fic_amd.encode_gray(lena64, B, wK, n_iso, search="lsq")
        assert_same(r, want, "fic_amd.encode_gray(search='lsq')")


def test_option_values(lena64):
    with fic_amd.Encoder(64, 64, 8, None, 1) as enc:
        enc.set_gray(lena64)
        enc.encode()
        with pytest.raises(fic_amd.FicError) as e:             # the last encode was a reference one
            enc.lsq_error()
        assert e.value.code == E_STATE
        enc.set_option("search", 1)
        for bad in (6, 3, 5, -1):
            with pytest.raises(fic_amd.FicError) as e:
                enc.set_option("sweep", bad)
            assert e.value.code == E_ARGUMENT
        with pytest.raises(fic_amd.FicError) as e:
            enc.set_option("search", 2)
        assert e.value.code == E_ARGUMENT
        enc.encode()                                            # the refused values changed nothing
        assert enc.last_kernel() == "k_sweep_lsq_fast"
        enc.set_option("search", "reference")
        enc.set_option("sweep", 6)
        with pytest.raises(fic_amd.FicError) as e:             # the other order
            enc.set_option("search", "lsq")
        assert e.value.code == E_ARGUMENT
        enc.encode()
        assert enc.info()["sweep_kind"] == 6
    with fic_amd.Encoder(64, 64, 8, 3, 1) as enc:               # a windowed search has no fast sweep
        enc.set_gray(lena64)
        enc.set_option("search", "lsq")
        enc.set_option("sweep", 2)
        with pytest.raises(fic_amd.FicError) as e:
            enc.encode()
        assert e.value.code == E_ARGUMENT


def test_streams_decoders_and_collage_lena64(lena64):
    B, n_iso = 4, 8
    h, w = lena64.shape
    wK = fo.geometry(w, h, B)[2]
    want = model("lena64", lena64, B, None, n_iso)
    ref = fo.decode_rows(want["qrows"], want["iso"], w, h, B, wK)
    with fic_amd.Encoder(w, h, B, None, n_iso) as enc:
        enc.set_option("search", "lsq")
        enc.set_gray(lena64)
        enc.encode()
        got = results(enc)
        assert_same(got, want, "lena64")
        run = fic_amd.write_run_gray_iso(got["qrows"], got["iso"], w, h, B, wK)
        img, avg, it = fic_amd.decode_gray_iso_run(run)
        assert (img == ref[0]).all() and avg.view(np.uint32) == ref[1].view(np.uint32) and it == ref[2]
        ctx_img, ctx_avg, ctx_it = enc.decode()
        assert (ctx_img[0] == ref[0]).all() and ctx_avg[0].view(np.uint32) == ref[1].view(np.uint32) and ctx_it[0] == ref[2]
        painted = gm.collage(lena64, B, want["idx_global"], want["a"], want["b"], want["iso"])[0]
        assert (enc.collage()[0] == painted).all()
    # what the search is for: a better decode than the reference criterion's rows at the same size
    r = fo.encode_gray(fo.gray_to_argb(lena64), w, h, B, wK, n_iso)
    old = fo.decode_rows(fo.quantise_gray(r["info"]), r["iso"], w, h, B, wK)[0]
    assert fo.psnr(img, lena64) > fo.psnr(old, lena64) + 1.0


QT_CASES = [(32, 32, 0), (32, 32, 1), (48, 32, 1)]


@pytest.mark.parametrize("n_iso", [1, 8])
@pytest.mark.parametrize("w,h,wK", QT_CASES, ids=[f"{c[0]}x{c[1]}-wK{c[2]}" for c in QT_CASES])
def test_quadtree_with_least_squares_levels(lena64, w, h, wK, n_iso):
    for g in (np.ascontiguousarray(lena64[8:8 + h, 4:4 + w]), clamp_image(w, h)):
        cbs = lm.codebooks(g, 16, 4, wK, n_iso)
        for t in (INF, 100.0, -1.0):
            want = qm.encode(g, 16, 4, wK, n_iso, t, cbs)
            leaves = fic_amd.encode_gray_quadtree(g, 16, 4, wK, n_iso, t, search="lsq")
            assert leaves.shape == want.shape and (leaves == want).all(), f"leaf table at threshold {t}"
            run = fic_amd.write_run_quadtree(leaves, w, h, 16, 4, wK, n_iso)
            assert run == qm.write_run(want, w, h, 16, 4, wK, n_iso)
            a, b = fic_amd.decode_quadtree_run(run), qm.decode(run)
            assert (a[0] == b[0]).all() and a[1].view(np.uint32) == b[1].view(np.uint32) and a[2] == b[2]
        twin = fic_amd.encode_gray_quadtree(fo.gray_to_argb(g).reshape(h, w), 16, 4, wK, n_iso, 100.0, search="lsq")
        assert (twin == qm.encode(g, 16, 4, wK, n_iso, 100.0, cbs)).all()
        # the reference entry on the same geometry afterwards: its own codebooks, as before
        ref = fic_amd.encode_gray_quadtree(g, 16, 4, wK, n_iso, 100.0)
        assert (ref == qm.encode(g, 16, 4, wK, n_iso, 100.0)).all()


def test_quadtree_refuses_what_the_reference_entry_refuses(lena64):
    g = np.ascontiguousarray(lena64[:32, :48])                  # full search at every level needs a square block grid
    codes = []
    for search in ("reference", "lsq"):
        with pytest.raises(fic_amd.FicError) as e:
            fic_amd.encode_gray_quadtree(g, 16, 4, 0, 1, 100.0, search=search)
        codes.append(e.value.code)
    assert codes[0] == codes[1]
