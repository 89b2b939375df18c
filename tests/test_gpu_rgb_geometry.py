"""The joint-RGB encoder (n_iso = 1 and 8) at the geometry edges, on the GPU against the CPU references, exactly: the minimum
geometries of tests/geomcases.py (Rw or Rh = 2, so Dw or Dh = 1; one column tile and a padded one in the 8-isometry matrix-core
mode at B = 16; W > H and H > W, where scaleImageRGB's `x + 1 >= height` quirk shows) and its seeded fuzz list (non-square
images, windows, batches of 1..3 different images, seven image kinds).  The reference is the oracle's encodeRGB / collage /
decodeRGB for n_iso = 1 and tests/rgbisomodel.py for n_iso = 8 (test_geometry_cases_model.py pins the two to each other).

Per case: the codebook (idx_local, iso, qrows; the float32 bits of a, bR, bG, bB) through the one-shot entry and through one
context, every collage pixel, the context's decode (pixels, alpha, avgError bits, iterations); automatic sweep always, and on
full-search cases the forced VALU and matrix-core sweeps with a drawn chunk count, the kernel asserted where include/fic.h
states the choice; then the same context takes a second set of images and everything runs again in another order, so the key
buffer, theta_g and the fragment stores of an earlier encode or sweep must not show.  The minimum geometries also decode at
zoom 2 against the stream models.  A failure names the case (its id rebuilds it), the sweep, the plane and the first range
block that differs."""
import numpy as np
import pytest

import fic_amd
import geomcases as gc
import isostreammodel as im
import zoommodel as zm

pytestmark = pytest.mark.gpu
CHUNKS = (0, 1, 2, 3, 7, 100000)


def _first(mask):
    j = np.flatnonzero(np.asarray(mask).reshape(-1))
    return int(j[0]) if j.size else None


def _bits_differ(x, y):
    """Per element: float32 bits differ, every NaN counted equal (conftest.same_f32, element-wise)."""
    x, y = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)
    nx, ny = np.isnan(x), np.isnan(y)
    return (nx != ny) | (~nx & ~ny & (x.view(np.uint32) != y.view(np.uint32)))


def _pixel_blocks(c, mask):
    """[h*w] pixel mask -> [N_r] range-block mask."""
    return mask.reshape(c.h // c.B, c.B, c.w // c.B, c.B).any(axis=(1, 3)).reshape(-1)


def _fail(where, what, j, got, want):
    raise AssertionError(f"{where}: {what} differs first at range block {j}: got {got}, reference {want}")


def _same_codebook(c, where, got, ref, collage=True):
    """got: dict of [N_r] arrays (+ collage [h*w]) of one plane."""
    j = _first(got["idx_local"] != ref["info"][:, 0].astype(np.int32))
    if j is not None:
        _fail(where, "idx_local", j, got["idx_local"][j], ref["info"][j, 0])
    j = _first(got["iso"] != ref["iso"])
    if j is not None:
        _fail(where, "iso", j, got["iso"][j], ref["iso"][j])
    for k, col in (("a", 1), ("bR", 2), ("bG", 3), ("bB", 4)):
        j = _first(_bits_differ(got[k], ref["info"][:, col]))
        if j is not None:
            _fail(where, f"{k} bits", j, got[k][j].view(np.uint32), ref["info"][j, col].view(np.uint32))
    j = _first((got["qrows"] != ref["qrows"]).any(axis=1))
    if j is not None:
        _fail(where, "qrows", j, got["qrows"][j], ref["qrows"][j])
    if collage:
        j = _first(_pixel_blocks(c, np.asarray(got["collage"]).reshape(-1) != ref["collage"].reshape(-1)))
        if j is not None:
            _fail(where, "collage", j, "", "")


def _same_decode(c, where, out, avg, it, want, z=1):
    """out: int32 ARGB [z*h * z*w] of one plane against (rgb uint8 [z*h, z*w, 3], avgError, iterations)."""
    zc = c._replace(w=z * c.w, h=z * c.h, B=z * c.B)
    u = np.asarray(out).reshape(-1).view(np.uint32)
    rgb = np.stack([(u >> 16) & 0xFF, (u >> 8) & 0xFF, u & 0xFF], axis=-1)
    j = _first(_pixel_blocks(zc, (rgb != want[0].reshape(-1, 3)).any(axis=1)))
    if j is not None:
        _fail(where, f"decode (zoom {z})", j, "", "")
    assert (u >> 24 == 0xFF).all(), f"{where}: decode (zoom {z}) alpha"
    assert np.float32(avg).view(np.uint32) == np.float32(want[1]).view(np.uint32) and int(it) == int(want[2]), \
        f"{where}: decode (zoom {z}) avgError {avg} after {it} iterations, reference {want[1]} after {want[2]}"


def _expect_kernel(c, where, enc, sweep):
    """The sweep policy of include/fic.h: the matrix-core mode for full search when asked for, and automatically when
    n_iso N_r N_d >= 3e7 or B = 16; else k_sweep_rgb_fast[_iso]<n> for full search at B = 4 / 8 and k_sweep_rgb[_iso]."""
    Rw, Rh, Dw, Dh = gc.dims(c)
    full = gc.is_full(c)
    use_q = full and (sweep == 2 or (sweep == 0 and (c.n_iso * Rw * Rh * Dw * Dh >= 3e7 or c.B == 16)))
    name, iso = enc.last_kernel(), "_iso" if c.n_iso == 8 else ""
    if use_q:
        NK, mode = c.B * c.B // 16, 4 if c.n_iso == 8 else 3
        assert enc.last_sweep() == 2 and name.startswith((f"k_sweep_q<{NK}, {mode}, ", f"k_sweep_qs<{NK}, {mode}>")), f"{where}: {name}"
    else:
        want = f"k_sweep_rgb_fast{iso}<{c.B * c.B}>" if full and c.B <= 8 else f"k_sweep_rgb{iso}"
        assert enc.last_sweep() == 1 and name == want, f"{where}: {name}, expected {want}"


def _zoom_reference(c, ref, z):
    if c.n_iso == 1:
        return zm.decode_rgb(zm.fixed_run(1, ref["qrows"], c.w, c.h, c.B, c.wK), z)
    return im.reference(im.write_fixed(5, ref["qrows"], ref["iso"], c.w, c.h, c.B, c.wK), z)


def _run_case(c, zoom2):
    cid = gc.case_id(c)
    rng = np.random.default_rng(c.seed)
    sweeps = [0, 1, 2] if gc.is_full(c) else [0]
    with fic_amd.capi.RgbEncoder(c.w, c.h, c.B, c.wK, planes=c.planes, n_iso=c.n_iso) as enc:
        for first in (0, 1):                               # images 0 .. planes - 1, then 1 .. planes on the same context
            argbs = gc.case_images(c, first)
            one = fic_amd.encode_rgb(argbs[0], c.w, c.h, c.B, c.wK, want_collage=True, n_iso=c.n_iso)
            _same_codebook(c, f"{cid} one-shot image {first}", one, gc.case_reference(c, first))
            enc.set_argb(argbs)
            for sweep in [sweeps[i] for i in rng.permutation(len(sweeps))]:
                chunks = int(rng.choice(CHUNKS)) if len(sweeps) > 1 else 0
                enc.set_option("sweep", sweep)
                enc.set_option("chunks", chunks)
                enc.encode(with_collage=True)
                res = enc.results()
                out, avg, it = enc.decode()
                for p in range(c.planes):
                    where = f"{cid} image set {first} sweep={sweep} chunks={chunks} plane {p}"
                    ref = gc.case_reference(c, first + p)
                    _same_codebook(c, where, {k: v[p] for k, v in res.items()}, ref)
                    _same_decode(c, where, out[p], avg[p], it[p], ref["decode"])
                _expect_kernel(c, f"{cid} sweep={sweep} chunks={chunks}", enc, sweep)
        if zoom2:                                          # the rows of the last encode (images 1 .. planes)
            out, avg, it = enc.decode(zoom=2)
            for p in range(c.planes):
                _same_decode(c, f"{cid} plane {p}", out[p], avg[p], it[p], _zoom_reference(c, gc.case_reference(c, 1 + p), 2), z=2)


@pytest.mark.parametrize("c", gc.MIN_CASES, ids=gc.case_id)
def test_minimum_geometry(c):
    _run_case(c, zoom2=True)


@pytest.mark.parametrize("c", gc.FUZZ_CASES, ids=gc.case_id)
def test_fuzz_case(c):
    _run_case(c, zoom2=False)


def test_b16_eight_isometries_is_the_matrix_core_mode_from_one_column_tile_up():
    """32 x 32 at B = 16 with 8 isometries: N_d = 1, N_r = 4, 32 columns -- exactly one column tile; 48 x 48 has 72 columns and a
    padded tile.  Automatic must be k_sweep_q<16, 4, ..> / k_sweep_qs<16, 4> even there (B = 16 has no VALU full-search kernel),
    whatever the chunk count asked for; what it computes is checked by test_minimum_geometry."""
    for w, wK in ((32, 1), (48, 3)):
        c = next(c for c in gc.MIN_CASES if (c.w, c.h, c.B, c.wK, c.n_iso) == (w, w, 16, wK, 8))
        with fic_amd.capi.RgbEncoder(c.w, c.h, 16, c.wK, planes=c.planes, n_iso=8) as enc:
            enc.set_argb(gc.case_images(c))
            for chunks in CHUNKS:
                enc.set_option("chunks", chunks)
                enc.encode()
                name = enc.last_kernel()
                assert enc.last_sweep() == 2 and name.startswith(("k_sweep_q<16, 4, ", "k_sweep_qs<16, 4>")), name
                res = enc.results()
                for p in range(c.planes):
                    _same_codebook(c, f"{gc.case_id(c)} chunks={chunks} plane {p}", {k: v[p] for k, v in res.items()},
                                   gc.case_reference(c, p), collage=False)
