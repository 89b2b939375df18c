"""Least-squares domain search of the joint-RGB path on the GPU (option "search" = 1 of a colour context:
k_sweep_lsq_rgb_generic / k_sweep_lsq_rgb_fast) against the numpy int64 model tests/rgblsqmodel.py, bit
for bit: idx_local, iso, qrows5, E and the bits of a, bR, bG, bB -- on minimum, non-square, windowed and ragged geometries,
through both sweeps and several pool chunk counts, on inputs that tie everywhere, clamp qa and drive t negative; batched planes;
the cached contexts' hygiene; the streams, the decoders and the collage on such a codebook; the two quadtree entries.  (The
pool index idx_global has no getter on a colour context; the collage, which paints through it, stands for it, on windowed
searches where it differs from idx_local.)"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geomcases as gc  # noqa: E402
import isostreammodel as im  # noqa: E402
import qtrgbmodel as qr  # noqa: E402
import rgbisomodel as rim  # noqa: E402
import rgblsqmodel as lm  # noqa: E402

import fic_amd  # noqa: E402
from fic_amd import capi  # noqa: E402
from conftest import same_f32  # noqa: E402
from oracle import fic_oracle as fo  # noqa: E402

pytestmark = pytest.mark.gpu
E_ARGUMENT, E_STATE = -3, -7
INF = float("inf")

# (w, h, B, wK or None for the full search, chunk counts of the fast sweep besides the automatic one)
GEOMS = [(8, 8, 4, None, ()), (16, 16, 4, None, ()), (32, 32, 8, None, ()), (32, 32, 16, None, ()), (64, 32, 16, 1, ()),
         (48, 48, 16, 3, ()), (64, 64, 4, None, (1, 3, 5)), (64, 64, 16, None, ()), (160, 160, 16, None, ()),
         (144, 144, 8, None, (2,))]
IDS = [f"{g[0]}x{g[1]}-B{g[2]}-wK{g[3] or 'full'}" for g in GEOMS]
FIELDS = ("idx_local", "iso", "qrows", "E")


def clamp_image(w, h, seed=3):
    """2 x 2 cells: R [[255, 0], [e, 255]], G and B [[0, 255], [255 - e, 0]], e in 0, 4 .. 40.  The range blocks have full
    contrast while the scaled image -- (p00 + p10 + 2 p01) / 4 per cell: 63 .. 83 in R, 171 .. 191 in G and B -- has almost
    none, so 1000 C / V lies far outside -1000 .. 1000; where qa = 1000 the G and B offsets (mean 122 - 181) are negative."""
    rng = np.random.RandomState(seed)
    img = np.zeros((h, w, 3), np.int64)
    for ch in range(3):
        e = 4 * rng.randint(0, 11, size=(h // 2, w // 2))
        if ch == 0:
            img[0::2, 0::2, ch] = 255
            img[1::2, 0::2, ch] = e
            img[1::2, 1::2, ch] = 255
        else:
            img[0::2, 1::2, ch] = 255
            img[1::2, 0::2, ch] = 255 - e
    return img.astype(np.uint8)


def images(w, h):
    y, x = np.mgrid[0:h, 0:w]
    rng = np.random.RandomState(1000 * w + h)
    anti = rng.randint(0, 256, size=(h, w))
    out = {"constant": np.full((h, w, 3), (77, 130, 9), np.uint8),
           "random": rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8),
           "anti": np.stack([anti, 255 - anti, np.full((h, w), 90)], axis=-1).astype(np.uint8),
           "clamp": clamp_image(w, h),
           "ramp": np.stack([x * 255 // max(w - 1, 1), y * 128 // max(h - 1, 1), 255 - (x + y) * 255 // max(w + h - 2, 1)], -1).astype(np.uint8)}
    for kind in ("U", "S", "low", "lena"):
        out[kind] = gc.rgb_image(kind, w, h, 31 + w + h, 0)
    return out


_MODEL = {}


def model(name, rgb, B, wK, n_iso):
    h, w = rgb.shape[:2]
    key = (name, w, h, B, wK, n_iso)
    if key not in _MODEL:
        _MODEL[key] = lm.encode(fo.rgb_to_argb(rgb), w, h, B, wK, n_iso)
    return _MODEL[key]


def assert_same(got, want, what):
    for f in FIELDS:
        assert (np.asarray(got[f]) == want[f]).all(), f"{what}: {f}"
    for f in ("a", "bR", "bG", "bB"):
        assert same_f32(got[f], want[f]), f"{what}: bits of {f}"


def results(enc, plane=0):
    r = {k: v[plane] for k, v in enc.results().items()}
    r["E"] = enc.lsq_error()[plane]
    return r


def kernel_name(B, n_iso, fast):
    if not fast:
        return "k_sweep_lsq_rgb_generic"
    return f"k_sweep_lsq_rgb_fast<{3 * B * B // 4}, {1 if n_iso == 1 else (8 if B == 4 else 2)}>"


@pytest.mark.parametrize("n_iso", [1, 8])
@pytest.mark.parametrize("w,h,B,wK,chunks", GEOMS, ids=IDS)
def test_codebook_is_the_models(w, h, B, wK, chunks, n_iso):
    Rw, Rh, Dw, Dh = fo.geometry(w, h, B)
    wk = Dw if wK is None else wK
    fast_ok = wk == Dw == Dh and B <= 8
    runs = [(1, 0), (0, 0)] + ([(2, 0)] + [(2, c) for c in chunks] if fast_ok else [])
    with capi.RgbEncoder(w, h, B, wk, n_iso=n_iso) as enc:
        enc.set_option("search", "lsq")
        for name, rgb in images(w, h).items():
            want = model(name, rgb, B, wK, n_iso)
            enc.set_argb(fo.rgb_to_argb(rgb))
            got = {}
            for sweep, c in runs:
                enc.set_option("sweep", sweep)
                enc.set_option("chunks", c)
                enc.encode()
                assert enc.last_kernel() == kernel_name(B, n_iso, sweep == 2 or (sweep == 0 and fast_ok))
                got[(sweep, c)] = results(enc)
                assert_same(got[(sweep, c)], want, f"{name}, sweep {sweep}, chunks {c}")
            for key in runs[1:]:                              # the two kernels agree with each other as well
                assert_same(got[key], got[runs[0]], f"{name}, {key} against the generic sweep")
            qa, t = want["qrows"][:, 1] // 1000, want["qrows"][:, 2:]
            if name == "constant":                            # every pair ties and V = 0: the first candidate wins
                assert (want["idx_local"] == 0).all() and (want["iso"] == 0).all() and (qa == 0).all()
            if name == "clamp" and (w, h, B) == (64, 64, 4):  # 841 nearly flat pool blocks: every row clamps, offsets below 0
                assert (np.abs(qa) == 1000).all() and (t < 0).sum() >= 100
        if not fast_ok:                                       # the fast sweep exists for the full search at B <= 8 only
            enc.set_option("sweep", 2)
            with pytest.raises(fic_amd.FicError) as e:
                enc.encode()
            assert e.value.code == E_ARGUMENT


def test_three_planes():
    for B, n_iso in ((4, 8), (8, 1), (16, 8)):
        w = h = 64
        names = ("random", "lena", "clamp")
        imgs = [images(w, h)[k] for k in names]
        want = [model(k, g, B, None, n_iso) for k, g in zip(names, imgs)]
        with capi.RgbEncoder(w, h, B, fo.geometry(w, h, B)[2], planes=3, n_iso=n_iso) as enc:
            enc.set_option("search", "lsq")
            enc.set_argb(np.stack([fo.rgb_to_argb(g) for g in imgs]))
            for sweep in (0, 1):
                enc.set_option("sweep", sweep)
                enc.encode()
                for p in range(3):
                    assert_same(results(enc, p), want[p], f"B={B}, plane {p}, sweep {sweep}")


# windowed searches, where the pool index differs from the window-local one (48 x 48 at wK = 3 is the whole 3 x 3 pool)
WINDOWED = [(64, 32, 16, 1), (48, 48, 16, 3), (64, 64, 8, 3), (64, 64, 4, 5), (96, 64, 8, 2)]


@pytest.mark.parametrize("n_iso", [1, 8])
@pytest.mark.parametrize("w,h,B,wK", WINDOWED, ids=[f"{g[0]}x{g[1]}-B{g[2]}-wK{g[3]}" for g in WINDOWED])
def test_windowed_collage_paints_through_idx_global(w, h, B, wK, n_iso):
    """A colour context has no getter for idx_global; k_collage_rgb reads it.  The collage of a windowed least-squares encode
    against rgbisomodel.collage of the model's rows, which resolves the window itself: a wrong pool index paints other pixels."""
    Dw = fo.geometry(w, h, B)[2]
    moved = 0
    with capi.RgbEncoder(w, h, B, wK, n_iso=n_iso) as enc:
        enc.set_option("search", "lsq")
        for name in ("random", "lena", "ramp"):
            rgb = images(w, h)[name]
            argb = fo.rgb_to_argb(rgb)
            want = model(name, rgb, B, wK, n_iso)
            moved += int((want["idx_global"] != want["idx_local"]).sum())
            info = np.stack([want["idx_local"].astype(np.float32), want["a"], want["bR"], want["bG"], want["bB"]], axis=1)
            painted = rim.collage(argb, w, h, B, wK, info, want["iso"])
            # the same rows painted as if idx_local were the pool index: must differ, or the comparison below shows nothing
            full = rim.collage(argb, w, h, B, Dw, info, want["iso"]) if wK != Dw else None
            enc.set_argb(argb)
            enc.encode(with_collage=True)
            got = results(enc)
            assert_same(got, want, f"{name}")
            assert (got["collage"] == painted).all(), name
            if full is not None and (want["idx_global"] != want["idx_local"]).any():
                assert (painted != full).any(), name
    if wK != Dw:
        assert moved > 0


def test_cached_contexts_stay_in_reference_mode(lena_colored):
    rgb = np.ascontiguousarray(lena_colored[96:160, 64:128])
    argb = fo.rgb_to_argb(rgb)
    for B, wK, n_iso in ((4, None, 1), (8, 3, 8)):
        wk = fo.geometry(64, 64, B)[2] if wK is None else wK
        before = fic_amd.encode_rgb(argb, 64, 64, B, wk, n_iso=n_iso)
        lsq = fic_amd.encode_rgb(argb, 64, 64, B, wk, n_iso=n_iso, search="lsq")
        after = fic_amd.encode_rgb(argb, 64, 64, B, wk, n_iso=n_iso)
        for k in ("idx_local", "iso", "qrows"):
            assert (before[k] == after[k]).all()
        for k in ("a", "bR", "bG", "bB"):
            assert same_f32(before[k], after[k])
        want = model("lena64", rgb, B, wK, n_iso)
        assert_same(lsq, want, "fic_encode_rgb_lsq_argb")
        assert not (lsq["qrows"] == before["qrows"]).all()


def test_option_values(lena_colored):
    argb = fo.rgb_to_argb(np.ascontiguousarray(lena_colored[:64, :64]))
    with capi.RgbEncoder(64, 64, 8, 13) as enc:
        enc.set_argb(argb)
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
        assert enc.last_kernel() == "k_sweep_lsq_rgb_fast<48, 1>"
        enc.lsq_error()
        enc.set_option("search", "reference")
        for bad in (6, 3):                                      # the other order: no value is good for one search only
            with pytest.raises(fic_amd.FicError) as e:
                enc.set_option("sweep", bad)
            assert e.value.code == E_ARGUMENT
        enc.set_option("search", "lsq")
        enc.set_option("search", "reference")
        enc.encode()
        assert enc.last_kernel() == "k_sweep_rgb_fast<64>"
        with pytest.raises(fic_amd.FicError) as e:
            enc.lsq_error()
        assert e.value.code == E_STATE


def _unpack(argb, w, h):
    return qr.channels(argb, w, h).astype(np.uint8)


def test_streams_decoders_and_collage_lena64(lena_colored):
    B, n_iso, w, h = 4, 8, 64, 64
    rgb = np.ascontiguousarray(lena_colored[96:160, 64:128])
    argb = fo.rgb_to_argb(rgb)
    wK = fo.geometry(w, h, B)[2]
    want = model("lena64", rgb, B, None, n_iso)
    ref = rim.decode(want["qrows"], want["iso"], w, h, B, wK)
    info = np.stack([want["idx_local"].astype(np.float32), want["a"], want["bR"], want["bG"], want["bB"]], axis=1)
    with capi.RgbEncoder(w, h, B, wK, n_iso=n_iso) as enc:
        enc.set_option("search", "lsq")
        enc.set_argb(argb)
        enc.encode(with_collage=True)
        got = results(enc)
        assert_same(got, want, "lena64")
        run = fic_amd.write_run_rgb_iso(got["qrows"], got["iso"], w, h, B, wK)
        out = fic_amd.decode_rgb_iso_run(run)
        assert (_unpack(out[0], w, h) == ref[0]).all() and same_f32(out[1], ref[1]) and int(out[2]) == ref[2]
        ctx_img, ctx_avg, ctx_it = enc.decode()
        assert (_unpack(ctx_img[0], w, h) == ref[0]).all() and same_f32(ctx_avg[0], ref[1]) and int(ctx_it[0]) == ref[2]
        assert (got["collage"] == rim.collage(argb, w, h, B, wK, info, want["iso"])).all()
    # what the search is for: a better decode than the reference criterion's rows at the same size
    r = rim.encode(argb, w, h, B, wK, n_iso)
    old = rim.decode(r["qrows"], r["iso"], w, h, B, wK)[0]
    assert fo.psnr(ref[0], rgb) > fo.psnr(old, rgb) + 1.0


QT_CASES = [(32, 32, 0), (32, 32, 1), (48, 32, 1)]


@pytest.mark.parametrize("n_iso", [1, 8])
@pytest.mark.parametrize("w,h,wK", QT_CASES, ids=[f"{c[0]}x{c[1]}-wK{c[2]}" for c in QT_CASES])
def test_quadtree_with_least_squares_levels(lena_colored, w, h, wK, n_iso):
    for rgb in (np.ascontiguousarray(lena_colored[100:100 + h, 60:60 + w]), clamp_image(w, h)):
        argb = fo.rgb_to_argb(rgb)
        cbs = lm.codebooks(argb, w, h, 16, 4, wK, n_iso)
        for t in (INF, 600.0, -1.0):
            want = im.encode(argb, w, h, 16, 4, wK, n_iso, t, cbs)
            leaves = fic_amd.encode_rgb_quadtree_iso(argb, w, h, 16, 4, wK, n_iso, t, search="lsq")
            assert leaves.shape == want.shape and (leaves == want).all(), f"tag 6 leaf table at threshold {t}"
            run = fic_amd.write_run_rgb_quadtree_iso(leaves, w, h, 16, 4, wK)
            assert run == im.write_qt(want, w, h, 16, 4, wK)
            a, b = fic_amd.decode_rgb_quadtree_iso_run(run), im.decode_qt(run)
            assert (_unpack(a[0], w, h) == b[0]).all() and same_f32(a[1], b[1]) and int(a[2]) == b[2]
            if n_iso == 1:                                      # tag 3: the same rows without the column
                want3 = qr.encode(argb, w, h, 16, 4, wK, t, {B: q for B, (q, _) in cbs.items()})
                leaves3 = fic_amd.encode_rgb_quadtree(argb, w, h, 16, 4, wK, t, search="lsq")
                assert leaves3.shape == want3.shape and (leaves3 == want3).all(), f"tag 3 leaf table at threshold {t}"
                run3 = fic_amd.write_run_rgb_quadtree(leaves3, w, h, 16, 4, wK)
                assert run3 == qr.write_run(want3, w, h, 16, 4, wK)
                a, b = fic_amd.decode_rgb_quadtree_run(run3), qr.decode(run3)
                assert (_unpack(a[0], w, h) == b[0]).all() and same_f32(a[1], b[1]) and int(a[2]) == b[2]
        # the reference entry on the same geometry afterwards: its own codebooks, as before
        ref = fic_amd.encode_rgb_quadtree_iso(argb, w, h, 16, 4, wK, n_iso, 600.0)
        assert (ref == im.encode(argb, w, h, 16, 4, wK, n_iso, 600.0)).all()
