"""The prune bound of k_sweep_lsq_rgb_fast on the GPU, on the inputs of tests/lsqtight.py:
  1. Tight colour images -- probe ranges whose winner clears |C'| <= li by a relative 2^-19 .. 2^-22 only
     (tests/test_lsq_bound.py) -- give the codebook of the numpy int64 model tests/rgblsqmodel.py bit for bit, in every fast
     instantiation, with one pool chunk, the automatic count and a count that cuts the pool between a near fit and its winner,
     against the generic sweep, and two different images in one context.  "sweep_stats" shows that the prune was at work.
  2. A bound too wide is CAUGHT: option "lsq_tau_widen" = WIDEN_CAUGHT (tau times 1 + 2^-17, the widening the model says the
     probes catch) changes probe rows; back at 0 the same context gives the model's codebook again.
  3. Full-range images (pixels 0 and 255) against the model: at B = 16, where V and |C| pass 2^31 and n S_dd wraps past 2^32,
     through the generic sweep -- full search and the windowed entry at wK = 3 --, at B = 8 and 4 through both sweeps."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lsqtight as lt  # noqa: E402
import rgblsqmodel as lm  # noqa: E402

import fic_amd  # noqa: E402
from fic_amd import capi  # noqa: E402
from conftest import same_f32  # noqa: E402
from oracle import fic_oracle as fo  # noqa: E402

pytestmark = pytest.mark.gpu
E_ARGUMENT = -3
CASES = list(lt.FAST[True])
IDS = [f"B{B}-iso{k}" for B, k in CASES]
FIELDS = ("idx_local", "iso", "qrows", "E")
GENERIC = "k_sweep_lsq_rgb_generic"

_MODEL = {}


def model(key, rgb, B, n_iso, wK=None):
    if key not in _MODEL:
        h, w = rgb.shape[:2]
        _MODEL[key] = lm.encode(fo.rgb_to_argb(rgb), w, h, B, wK, n_iso)
    return _MODEL[key]


def tight_model(B, n_iso, seed):
    img, table = lt.tight_rgb(B, n_iso, seed)
    return img, table, model(("tight", B, n_iso, seed), img, B, n_iso)


def fast_name(B, n_iso):
    return f"k_sweep_lsq_rgb_fast<{3 * B * B // 4}, {lt.FAST[True][(B, n_iso)][1]}>"


def assert_same(got, want, what):
    for f in FIELDS:
        assert (np.asarray(got[f]) == want[f]).all(), f"{what}: {f}"
    for f in ("a", "bR", "bG", "bB"):
        assert same_f32(got[f], want[f]), f"{what}: bits of {f}"


def results(enc, plane=0):
    r = {k: v[plane] for k, v in enc.results().items()}
    r["E"] = enc.lsq_error()[plane]
    return r


def rows_that_differ(got, want, rows):
    rows = np.asarray(rows)
    bad = np.zeros(rows.size, bool)
    for f in ("idx_local", "iso", "E"):
        bad |= np.asarray(got[f])[rows] != want[f][rows]
    return {int(j) for j in rows[bad]}


def encoder(w, B, n_iso, planes=1, wK=None):
    return capi.RgbEncoder(w, w, B, fo.geometry(w, w, B)[2] if wK is None else wK, planes=planes, n_iso=n_iso)


@pytest.mark.parametrize("B,n_iso", CASES, ids=IDS)
def test_tight_codebooks_are_the_models(B, n_iso):
    W = lt.SIDE[B]
    (img1, table, want1), (img2, _, want2) = tight_model(B, n_iso, 1), tight_model(B, n_iso, 2)
    cut = lt.cutting_chunks(B, table, True)
    with encoder(W, B, n_iso, planes=2) as enc:
        enc.set_option("search", "lsq")
        enc.set_argb(np.stack([fo.rgb_to_argb(img1), fo.rgb_to_argb(img2)]))
        for sweep, chunks in ((2, 1), (2, 0), (0, 0), (2, cut), (1, 0)):
            enc.set_option("sweep", sweep)
            enc.set_option("chunks", chunks)
            enc.encode()
            assert enc.last_kernel() == (GENERIC if sweep == 1 else fast_name(B, n_iso))
            for plane, want in enumerate((want1, want2)):
                assert_same(results(enc, plane), want, f"plane {plane}, sweep {sweep}, chunks {chunks}")


@pytest.mark.parametrize("B,n_iso", CASES, ids=IDS)
def test_the_prune_was_at_work(B, n_iso):
    W = lt.SIDE[B]
    img, table, want = tight_model(B, n_iso, 1)
    NC = lt.FAST[True][(B, n_iso)][1]
    with encoder(W, B, n_iso) as enc:
        enc.set_option("search", "lsq")
        enc.set_option("sweep", 2)
        enc.set_option("chunks", 1)
        enc.set_option("sweep_stats", 1)
        enc.set_argb(fo.rgb_to_argb(img))
        enc.encode()
        assert enc.last_kernel() == fast_name(B, n_iso)
        st = enc.sweep_stats()
        assert_same(results(enc), want, "with sweep_stats")
        nd = fo.geometry(W, W, B)[2] ** 2
        pairs = enc.n_ranges * nd * n_iso
        print(f"\n[rgb lsq prune] B={B} n_iso={n_iso}: {st['exact_pairs']} of {pairs} pairs evaluated exactly, "
              f"{st['flagged_tiles']} of {st['tiles']} (wave, pool block) visits ran the epilogue, {st['waves']} waves")
        assert 0 < st["exact_pairs"] < pairs
        assert st["waves"] == (enc.n_ranges + 63) // 64 * (n_iso // NC)
        assert 0 < st["flagged_tiles"] <= st["tiles"] == st["waves"] * nd


@pytest.mark.parametrize("B,n_iso", CASES, ids=IDS)
def test_a_bound_too_wide_is_caught(B, n_iso):
    """tau times 1 + 2^-WIDEN_CAUGHT: the model (lsqtight.li_model on the probe table) says that a quarter of the probes or more
    lose their winner to a wrong skip.  One pool chunk, so that every probe has its near fit ahead of its winner."""
    W = lt.SIDE[B]
    img, table, want = tight_model(B, n_iso, 1)
    probes = [p["j"] for p in table]
    k = lt.WIDEN_CAUGHT[(True, B, n_iso)]
    with encoder(W, B, n_iso) as enc:
        enc.set_option("search", "lsq")
        enc.set_option("sweep", 2)
        enc.set_option("chunks", 1)
        enc.set_argb(fo.rgb_to_argb(img))
        enc.set_option("lsq_tau_widen", k)
        enc.encode()
        assert enc.last_kernel() == fast_name(B, n_iso)
        wide = results(enc)
        bad = rows_that_differ(wide, want, probes)
        # the model's forecast, probe by probe: li with the widened tau reaches |C'|.  Every probe is a relative 2^-20 or more
        # away from the edge of that forecast, a few ulp of an f32: a sqrtf that is one ulp off would not move it
        li = lt.li_model([p["Ti"] for p in table], [p["V"] for p in table], k, True)
        forecast = {p["j"] for l, p in zip(li, table) if int(l) >= abs(p["C"])}
        print(f"\n[rgb lsq_tau_widen] B={B} n_iso={n_iso}: {len(bad)} of {len(probes)} probe rows differ at k = {k}, forecast {len(forecast)}")
        assert len(bad) >= 1 and len(forecast) * 4 >= len(probes)
        assert bad == forecast
        assert (wide["E"][probes] >= want["E"][probes]).all()        # a wrong skip can only lose the best candidate
        enc.set_option("lsq_tau_widen", 0)
        enc.encode()
        assert_same(results(enc), want, "lsq_tau_widen back at 0")
        enc.set_option("sweep", 1)                                    # the generic sweep has no bound to widen
        enc.set_option("lsq_tau_widen", k)
        enc.encode()
        assert enc.last_kernel() == GENERIC
        assert_same(results(enc), want, "generic sweep under lsq_tau_widen")


def test_lsq_tau_widen_is_range_checked():
    with encoder(64, 4, 1) as enc:
        for bad in (-1, 1, 7, 25, 100):
            with pytest.raises(fic_amd.FicError) as e:
                enc.set_option("lsq_tau_widen", bad)
            assert e.value.code == E_ARGUMENT
        for ok in (8, 24, 0):
            enc.set_option("lsq_tau_widen", ok)


FULL_IDS = [f"{c[0]}-B{c[1]}-{'equal' if c[2] else 'free'}" for c in lt.RGB_FULL]


@pytest.mark.parametrize("n_iso", [1, 8])
@pytest.mark.parametrize("w,B,equal,perturb", lt.RGB_FULL, ids=FULL_IDS)
def test_full_range_images(w, B, equal, perturb, n_iso):
    img = lt.halves_image(w, w, B, 3, lt.HALVES_SEED, equal=equal, perturb=perturb)
    wK = 3 if w == 48 else None                                       # 48 x 48 at B = 16: the 3 x 3 pool through the windowed entry
    want = model(("halves", w, B, equal, n_iso), img, B, n_iso, wK)
    assert (want["E"] > 0).mean() >= 0.25                             # the comparison of qa, t and E means something
    fast = B <= 8
    with encoder(w, B, n_iso, wK=wK) as enc:
        enc.set_option("search", "lsq")
        enc.set_argb(fo.rgb_to_argb(img))
        for sweep, chunks in ((0, 0), (1, 0)) + (((2, 1),) if fast else ()):
            enc.set_option("sweep", sweep)
            enc.set_option("chunks", chunks)
            enc.encode()
            assert enc.last_kernel() == (fast_name(B, n_iso) if fast and sweep != 1 else GENERIC)
            assert_same(results(enc), want, f"sweep {sweep}, chunks {chunks}")
