"""Joint-RGB encode, collage and decode with the 8 isometries of the square on the GPU (fic_encode_rgb_iso_argb,
fic_rgb_ctx_create_iso) against the numpy model tests/rgbisomodel.py, exactly: candidate, isometry, the
float32 bits of a / bR / bG / bB, the quantised rows, every collage and decoded pixel, avgError's bits and the iteration count.
With n_iso = 1 the new entries give the bits of their existing twins."""
import numpy as np
import pytest

import fic_amd
import rgbisomodel as rm
from conftest import same_f32

pytestmark = pytest.mark.gpu
E_GEOMETRY, E_WINDOW, E_ARGUMENT = -1, -2, -3


def _argb(oracle, rgb):
    return oracle.rgb_to_argb(np.ascontiguousarray(rgb, np.uint8))


def _crop(lena_colored, w, h, x0=64, y0=96):
    return lena_colored[y0:y0 + h, x0:x0 + w]


def _noise(w, h, seed):
    """Colour noise over the whole range: |greyR greyD| sums leave 2^24 at B = 8 / 16, so the accumulation order shows."""
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)


def _unpack(argb, w, h):
    u = np.asarray(argb).reshape(h, w).view(np.uint32)
    return np.stack([(u >> 16) & 0xFF, (u >> 8) & 0xFF, u & 0xFF], axis=-1).astype(np.uint8)


def _same_codebook(got, ref, plane=None):
    g = got if plane is None else {k: v[plane] for k, v in got.items()}
    assert (g["idx_local"] == ref["info"][:, 0].astype(np.int32)).all()
    assert (g["iso"] == ref["iso"]).all()
    for k, col in (("a", 1), ("bR", 2), ("bG", 3), ("bB", 4)):
        assert same_f32(g[k], ref["info"][:, col]), k
    assert (g["qrows"] == ref["qrows"]).all()


def _check(oracle, rgb, B, wK, kernel=None, sweep=None, chunks=None):
    """One image through the one-shot entry and through a context (collage, decode), everything against the model.  kernel: the
    name last_kernel must report ("k_sweep_q": any instantiation of the matrix-core 8-isometry mode <NK, 4>)."""
    h, w = rgb.shape[:2]
    argb = _argb(oracle, rgb)
    ref = rm.encode(argb, w, h, B, wK, 8)
    got = fic_amd.encode_rgb(argb, w, h, B, wK, want_collage=True, n_iso=8)
    _same_codebook(got, ref)
    rcol = rm.collage(argb, w, h, B, wK, ref["info"], ref["iso"])
    assert (got["collage"] == rcol).all()
    with fic_amd.capi.RgbEncoder(w, h, B, wK, n_iso=8) as enc:
        if sweep is not None:
            enc.set_option("sweep", sweep)
        if chunks is not None:
            enc.set_option("chunks", chunks)
        enc.set_argb(argb)
        enc.encode(with_collage=True)
        res = enc.results()
        _same_codebook(res, ref, 0)
        assert (res["collage"][0] == rcol).all()
        if kernel == "k_sweep_q":
            name, NK = enc.last_kernel(), B * B // 16
            assert name.startswith((f"k_sweep_q<{NK}, 4, ", f"k_sweep_qs<{NK}, 4>")) and enc.last_sweep() == 2, name
        elif kernel is not None:
            assert enc.last_kernel() == kernel and enc.last_sweep() == 1
        out, avg, it = enc.decode()
    img, ravg, rit = rm.decode(ref["qrows"], ref["iso"], w, h, B, wK)
    assert (_unpack(out[0], w, h) == img).all()
    assert same_f32(avg[0], ravg) and int(it[0]) == rit
    return got


@pytest.mark.parametrize("B,wK", [(4, 2), (4, 4), (4, 8), (8, 2), (8, 4), (8, 8), (16, 2), (16, 4), (16, 8)])
def test_windowed_search(lena_colored, oracle, B, wK):
    got = _check(oracle, _crop(lena_colored, 128, 128), B, wK, kernel="k_sweep_rgb_iso")
    assert (got["iso"] != 0).any()


@pytest.mark.parametrize("size,B,valu", [(64, 4, "k_sweep_rgb_fast_iso<16>"), (128, 8, "k_sweep_rgb_fast_iso<64>"),
                                         (128, 16, "k_sweep_rgb_iso")])
@pytest.mark.parametrize("sweep", [None, 1, 2])
def test_full_search(lena_colored, oracle, size, B, valu, sweep):
    """Each sweep forced, and automatic: 8 N_r N_d is below 3e7 at these sizes, so automatic is the VALU full-search kernel at
    B = 4 / 8 and the matrix-core mode k_sweep_q<16, 4> at B = 16."""
    Dw = fic_amd.geometry(size, size, B)[2]
    kernel = "k_sweep_q" if sweep == 2 or (sweep is None and B == 16) else valu
    got = _check(oracle, _crop(lena_colored, size, size), B, Dw, kernel=kernel, sweep=sweep)
    assert (got["iso"] != 0).any()


@pytest.mark.parametrize("B,chunks", [(4, 1), (4, 3), (8, 1), (8, 2), (8, 100000), (16, 1), (16, 5)])
def test_matrix_core_pool_chunks(lena_colored, oracle, B, chunks):
    """One pool chunk, a few, and a chunk per unrolled step (k_sweep_qs): the codebook does not depend on the chunking."""
    size = 64 if B == 4 else 128
    Dw = fic_amd.geometry(size, size, B)[2]
    _check(oracle, _crop(lena_colored, size, size), B, Dw, kernel="k_sweep_q", sweep=2, chunks=chunks)


@pytest.mark.parametrize("B,wK", [(8, 13), (16, 5), (4, 29)])
def test_matrix_core_on_noise_flat_and_odd_range_counts(oracle, B, wK):
    """Full-range noise (the exact evaluation's order shows), a flat image (only candidate (0, 0) can win) and 72 x 72 at B = 8
    (81 range blocks = 648 columns: the last column tile is partly padding) through the matrix-core mode."""
    _check(oracle, _noise(64, 64, 40 + B), B, wK, kernel="k_sweep_q", sweep=2)
    flat = np.empty((64, 64, 3), np.uint8)
    flat[:] = (90, 140, 33)
    got = _check(oracle, flat, B, wK, kernel="k_sweep_q", sweep=2)
    assert (got["idx_local"] == 0).all() and (got["iso"] == 0).all()
    if B == 8:
        _check(oracle, _noise(72, 72, 3), 8, fic_amd.geometry(72, 72, 8)[2], kernel="k_sweep_q", sweep=2)


def test_automatic_sweep_follows_the_pair_count(lena_colored, oracle):
    """256 x 256 at B = 8: 8 N_r N_d = 3.05e7 >= 3e7, so automatic is the matrix-core mode (with n_iso = 1 the same image is
    far below the threshold and stays on the VALU sweep); FIC_RGB_SWEEP-style forcing is the option "sweep"."""
    argb = _argb(oracle, lena_colored)
    with fic_amd.capi.RgbEncoder(256, 256, 8, 61, n_iso=8) as enc:
        enc.set_argb(argb)
        enc.encode()
        assert enc.last_sweep() == 2 and enc.last_kernel().startswith(("k_sweep_q<4, 4, ", "k_sweep_qs<4, 4>"))
        auto = enc.results()
        enc.set_option("sweep", 1)
        enc.encode()
        assert enc.last_sweep() == 1 and enc.last_kernel() == "k_sweep_rgb_fast_iso<64>"
        valu = enc.results()
    for k in auto:
        assert (auto[k].view(np.uint32) == valu[k].view(np.uint32)).all(), k
    with fic_amd.capi.RgbEncoder(256, 256, 8, 61, n_iso=1) as enc:
        enc.set_argb(argb)
        enc.encode()
        assert enc.last_sweep() == 1


def test_full_search_ranges_not_a_multiple_of_64(oracle):
    """72 x 72 at B = 8: 81 range blocks, so the second wave of k_sweep_rgb_fast_iso has 47 shadow lanes."""
    Dw = fic_amd.geometry(72, 72, 8)[2]
    _check(oracle, _noise(72, 72, 3), 8, Dw, kernel="k_sweep_rgb_fast_iso<64>")


@pytest.mark.parametrize("w,h,B,wK", [(128, 64, 8, 4), (64, 128, 8, 4), (128, 64, 4, 2), (64, 128, 16, 3)])
def test_non_square(lena_colored, oracle, w, h, B, wK):
    _check(oracle, _crop(lena_colored, w, h), B, wK)


@pytest.mark.parametrize("B,wK", [(4, 29), (8, 13), (16, 5), (8, 3)])
def test_colour_noise_where_the_order_matters(oracle, B, wK):
    """kovarianz leaves 2^24 on full-range noise at B = 8 / 16: a range-copy order or a tree sum would give other bits."""
    _check(oracle, _noise(64, 64, 40 + B), B, wK)


@pytest.mark.parametrize("B,wK", [(4, 29), (8, 13), (8, 2), (16, 3)])
def test_flat_image_takes_the_first_candidate(oracle, B, wK):
    """Every error is 0: the strict '<' keeps candidate 0 at isometry 0 everywhere."""
    rgb = np.empty((64, 64, 3), np.uint8)
    rgb[:] = (90, 140, 33)
    got = _check(oracle, rgb, B, wK)
    assert (got["idx_local"] == 0).all() and (got["iso"] == 0).all()


@pytest.mark.parametrize("B,wK", [(4, 29), (8, 13), (8, 4)])
def test_symmetric_blocks_tie_to_the_lowest_isometry(oracle, B, wK):
    """An image of 16 x 16 cells, each an 8 x 8 pattern symmetric under all 8 isometries of its centre (a function of the sorted
    distances to the mid lines) drawn with 2 x 2 pixels per element, so scaleImageRGB returns the pattern itself.  The domain
    blocks centred in a cell are symmetric, their 8 isometries tie exactly and k must be the lowest; whatever else ties, the
    model's lower (c, k) is the answer."""
    rng = np.random.RandomState(9)
    t = np.abs(np.arange(8) - 3.5).astype(np.int64)                   # 3 .. 0 0 .. 3
    lo, hi = np.minimum(t[:, None], t[None, :]), np.maximum(t[:, None], t[None, :])
    rgb = np.zeros((64, 64, 3), np.uint8)
    for cy in range(4):
        for cx in range(4):
            lut = rng.randint(0, 256, size=(4, 4, 3))
            rgb[16 * cy:16 * cy + 16, 16 * cx:16 * cx + 16] = np.repeat(np.repeat(lut[lo, hi], 2, axis=0), 2, axis=1)
    got = _check(oracle, rgb, B, wK)
    ref1 = rm.encode(_argb(oracle, rgb), 64, 64, B, wK, 1)
    tied = np.frombuffer(rm.encode(_argb(oracle, rgb), 64, 64, B, wK, 8)["err"].tobytes(), np.uint32) == \
        np.frombuffer(ref1["err"].tobytes(), np.uint32)
    assert tied.any()                                                 # ranges no isometry improves: they must keep (c, 0)
    keep = tied & (got["idx_local"] == ref1["info"][:, 0].astype(np.int32))
    assert keep.any() and (got["iso"][keep] == 0).all()


def test_three_plane_context(lena_colored, oracle):
    """Three different images in one context: windowed and full search, collage and decode per plane."""
    for B, wK in ((8, 4), (8, 29)):
        rgbs = [_crop(lena_colored, 128, 128), _noise(128, 128, 7), _crop(lena_colored, 128, 128, 0, 0)]
        if wK == 29:
            rgbs = [r[:64, :64] for r in rgbs]
            wK = fic_amd.geometry(64, 64, B)[2]
        h, w = rgbs[0].shape[:2]
        argbs = np.stack([_argb(oracle, r) for r in rgbs])
        with fic_amd.capi.RgbEncoder(w, h, B, wK, planes=3, n_iso=8) as enc:
            enc.set_argb(argbs)
            enc.encode(with_collage=True)
            res = enc.results()
            out, avg, it = enc.decode()
        for p in range(3):
            ref = rm.encode(argbs[p], w, h, B, wK, 8)
            _same_codebook(res, ref, p)
            assert (res["collage"][p] == rm.collage(argbs[p], w, h, B, wK, ref["info"], ref["iso"])).all()
            img, ravg, rit = rm.decode(ref["qrows"], ref["iso"], w, h, B, wK)
            assert (_unpack(out[p], w, h) == img).all()
            assert same_f32(avg[p], ravg) and int(it[p]) == rit


@pytest.mark.parametrize("B,wK", [(8, 2), (8, 61), (4, 4), (16, 29), (16, 2)])
def test_one_isometry_entries_equal_their_twins(lena_colored, oracle, B, wK):
    """fic_encode_rgb_iso_argb(n_iso = 1) and an n_iso = 1 context from fic_rgb_ctx_create_iso against the oracle's encodeRGB --
    what fic_encode_rgb_argb is pinned to -- with iso = 0 everywhere; the decode equals fo_decode_rgb."""
    argb = _argb(oracle, lena_colored)
    ref = oracle.encode_rgb(argb, 256, 256, B, wK)
    got = fic_amd.encode_rgb(argb, 256, 256, B, wK, want_collage=True, n_iso=1)
    with fic_amd.capi.RgbEncoder(256, 256, B, wK, n_iso=1) as enc:
        enc.set_argb(argb)
        enc.encode(with_collage=True)
        res = {k: v[0] for k, v in enc.results().items()}
        out, avg, it = enc.decode()
    for g in (got, res):
        assert (g["idx_local"] == ref[:, 0].astype(np.int32)).all() and (g["iso"] == 0).all()
        for k, col in (("a", 1), ("bR", 2), ("bG", 3), ("bB", 4)):
            assert same_f32(g[k], ref[:, col]), k
        assert (g["qrows"] == oracle.quantise_rgb(ref)).all()
        assert (g["collage"] == oracle.collage_rgb(argb, 256, 256, B, wK, ref)).all()
    rimg, ravg, rit = oracle.decode_rgb(oracle.write_run_rgb(ref, 256, 256, B, wK))
    assert (_unpack(out[0], 256, 256) == rimg).all() and same_f32(avg[0], ravg) and int(it[0]) == rit


def test_full_search_512_valu_against_matrix_cores(lena_colored, oracle):
    """Lena colour tiled to 512 x 512, B = 8, full search (15 625 domain blocks x 8 isometries per range block): the CPU model
    is too slow for the whole codebook, so the forced VALU sweep and the forced matrix-core sweep check each other on every
    row, collage and decode included, and the model checks a sample of rows spread over the image; every isometry occurs."""
    rgb = np.tile(lena_colored, (2, 2, 1))
    argb = _argb(oracle, rgb)
    Dw = fic_amd.geometry(512, 512, 8)[2]
    res = {}
    for sweep in (1, 2):
        with fic_amd.capi.RgbEncoder(512, 512, 8, Dw, n_iso=8) as enc:
            enc.set_option("sweep", sweep)
            enc.set_argb(argb)
            enc.encode(with_collage=True)
            assert enc.last_sweep() == sweep
            assert enc.last_kernel().startswith(("k_sweep_q<4, 4, ", "k_sweep_qs<4, 4>") if sweep == 2 else "k_sweep_rgb_fast_iso<64>")
            res[sweep] = {k: v[0].copy() for k, v in enc.results().items()}
            res[sweep]["decoded"], res[sweep]["avg"], res[sweep]["it"] = enc.decode()
    for k in res[1]:
        assert (np.asarray(res[1][k]).view(np.uint32) == np.asarray(res[2][k]).view(np.uint32)).all(), k
    got = res[2]
    rows = np.arange(5, 4096, 131)
    ref = rm.encode(argb, 512, 512, 8, Dw, 8, rows=rows)
    assert (got["idx_local"][rows] == ref["info"][rows, 0].astype(np.int32)).all()
    assert (got["iso"][rows] == ref["iso"][rows]).all()
    for k, col in (("a", 1), ("bR", 2), ("bG", 3), ("bB", 4)):
        assert same_f32(got[k][rows], ref["info"][rows, col]), k
    assert (got["qrows"][rows] == ref["qrows"][rows]).all()
    assert set(np.unique(got["iso"])) == set(range(8))


def test_error_codes(oracle):
    argb = _argb(oracle, _noise(64, 64, 1))
    for n_iso in (0, 2, 4, 9, -1):
        with pytest.raises(fic_amd.FicError) as e:
            fic_amd.encode_rgb(argb, 64, 64, 8, 2, n_iso=n_iso)
        assert e.value.code == E_ARGUMENT
        with pytest.raises(fic_amd.FicError) as e:
            fic_amd.capi.RgbEncoder(64, 64, 8, 2, n_iso=n_iso)
        assert e.value.code == E_ARGUMENT
    with pytest.raises(fic_amd.FicError) as e:                        # n_iso is checked first, the geometry next
        fic_amd.capi.RgbEncoder(64, 64, 8, 99, n_iso=8)
    assert e.value.code == E_WINDOW
    with fic_amd.capi.RgbEncoder(64, 64, 8, 13, n_iso=8) as enc:
        for name, value in (("sweep", 3), ("sweep", -1), ("chunks", -1), ("q_eshift", 5), ("no_such_option", 0)):
            with pytest.raises(fic_amd.FicError) as e:
                enc.set_option(name, value)
            assert e.value.code == E_ARGUMENT
        for value in (2, 1, 0):
            enc.set_option("sweep", value)
