"""The prune bound of k_sweep_lsq_fast on the GPU, on the inputs of tests/lsqtight.py:
  1. Tight images -- probe ranges whose winner clears |C'| <= li by a relative 2^-18 .. 2^-23 only (tests/test_lsq_bound.py) --
     give the codebook of the numpy int64 model tests/lsqmodel.py bit for bit, in every fast instantiation, with one pool chunk,
     the automatic count and a count that cuts the pool between a near fit and its winner, against the generic sweep, and two
     different images in one context.  "sweep_stats" shows that the prune was at work.
  2. A bound too wide is CAUGHT: option "lsq_tau_widen" = WIDEN_CAUGHT (tau times 1 + 2^-17, the widening the model says the
     probes catch) changes probe rows; back at 0 the same context gives the model's codebook again.
  3. Full-range images (pixels 0 and 255: R, V and |C| near their largest values) through both sweeps against the model."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lsqmodel as lm  # noqa: E402
import lsqtight as lt  # noqa: E402

import fic_amd  # noqa: E402
from conftest import same_f32  # noqa: E402

pytestmark = pytest.mark.gpu
E_ARGUMENT = -3
CASES = list(lt.FAST[False])
IDS = [f"B{B}-iso{k}" for B, k in CASES]
FIELDS = ("idx_local", "idx_global", "iso", "qrows", "E")
FAST, GENERIC = "k_sweep_lsq_fast", "k_sweep_lsq_generic"

_MODEL = {}


def model(key, img, B, n_iso):
    if key not in _MODEL:
        _MODEL[key] = lm.encode(img, B, None, n_iso)
    return _MODEL[key]


def tight_model(B, n_iso, seed):
    img, table = lt.tight_gray(B, n_iso, seed)
    return img, table, model(("tight", B, n_iso, seed), img, B, n_iso)


def assert_same(got, want, what):
    for f in FIELDS:
        assert (np.asarray(got[f]) == want[f]).all(), f"{what}: {f}"
    for f in ("a", "b", "err"):
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


@pytest.mark.parametrize("B,n_iso", CASES, ids=IDS)
def test_tight_codebooks_are_the_models(B, n_iso):
    W = lt.SIDE[B]
    (img1, table, want1), (img2, _, want2) = tight_model(B, n_iso, 1), tight_model(B, n_iso, 2)
    cut = lt.cutting_chunks(B, table, False)
    with fic_amd.Encoder(W, W, B, None, n_iso, planes=2) as enc:
        enc.set_option("search", "lsq")
        enc.set_gray(np.stack([img1, img2]))
        for sweep, chunks in ((2, 1), (2, 0), (0, 0), (2, cut), (1, 0)):
            enc.set_option("sweep", sweep)
            enc.set_option("chunks", chunks)
            enc.encode()
            assert enc.last_kernel() == (GENERIC if sweep == 1 else FAST)
            if chunks and sweep == 2:
                assert enc.info()["chunks"] == len(lt.chunk_starts(enc.n_domains, chunks, False))
            for plane, want in enumerate((want1, want2)):
                assert_same(results(enc, plane), want, f"plane {plane}, sweep {sweep}, chunks {chunks}")


@pytest.mark.parametrize("B,n_iso", CASES, ids=IDS)
def test_the_prune_was_at_work(B, n_iso):
    W = lt.SIDE[B]
    img, table, want = tight_model(B, n_iso, 1)
    with fic_amd.Encoder(W, W, B, None, n_iso) as enc:
        enc.set_option("search", "lsq")
        enc.set_option("sweep", 2)
        enc.set_option("chunks", 1)
        enc.set_option("sweep_stats", 1)
        enc.set_gray(img)
        enc.encode()
        assert enc.last_kernel() == FAST
        st = enc.sweep_stats()
        assert_same(results(enc), want, "with sweep_stats")
        pairs = enc.n_ranges * enc.n_domains * n_iso
        print(f"\n[lsq prune] B={B} n_iso={n_iso}: {st['exact_pairs']} of {pairs} pairs evaluated exactly, "
              f"{st['flagged_tiles']} of {st['tiles']} (wave, pool block) visits ran the epilogue, {st['waves']} waves")
        assert 0 < st["exact_pairs"] < pairs
        assert 0 < st["flagged_tiles"] <= st["tiles"] == st["waves"] * enc.n_domains


@pytest.mark.parametrize("B,n_iso", CASES, ids=IDS)
def test_a_bound_too_wide_is_caught(B, n_iso):
    """tau times 1 + 2^-WIDEN_CAUGHT: the model (lsqtight.li_model on the probe table) says that a quarter of the probes or more
    lose their winner to a wrong skip.  One pool chunk, so that every probe has its near fit ahead of its winner."""
    W = lt.SIDE[B]
    img, table, want = tight_model(B, n_iso, 1)
    probes = [p["j"] for p in table]
    k = lt.WIDEN_CAUGHT[(False, B, n_iso)]
    with fic_amd.Encoder(W, W, B, None, n_iso) as enc:
        enc.set_option("search", "lsq")
        enc.set_option("sweep", 2)
        enc.set_option("chunks", 1)
        enc.set_gray(img)
        enc.set_option("lsq_tau_widen", k)
        enc.encode()
        assert enc.last_kernel() == FAST
        wide = results(enc)
        bad = rows_that_differ(wide, want, probes)
        # the model's forecast, probe by probe: li with the widened tau reaches |C'|.  Every probe is a relative 2^-20 or more
        # away from the edge of that forecast, a few ulp of an f32: a sqrtf that is one ulp off would not move it
        li = lt.li_model([p["Ti"] for p in table], [p["V"] for p in table], k, False)
        forecast = {p["j"] for l, p in zip(li, table) if int(l) >= abs(p["C"])}
        print(f"\n[lsq_tau_widen] B={B} n_iso={n_iso}: {len(bad)} of {len(probes)} probe rows differ at k = {k}, forecast {len(forecast)}")
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
    with fic_amd.Encoder(64, 64, 4, None, 1) as enc:
        for bad in (-1, 1, 7, 25, 100):
            with pytest.raises(fic_amd.FicError) as e:
                enc.set_option("lsq_tau_widen", bad)
            assert e.value.code == E_ARGUMENT
        for ok in (8, 24, 0):
            enc.set_option("lsq_tau_widen", ok)


@pytest.mark.parametrize("n_iso", [1, 8])
@pytest.mark.parametrize("w,B,perturb", lt.GRAY_FULL, ids=[f"{c[0]}-B{c[1]}" for c in lt.GRAY_FULL])
def test_full_range_images(w, B, perturb, n_iso):
    img = lt.halves_image(w, w, B, 1, lt.HALVES_SEED, perturb=perturb)
    want = model(("halves", w, B, n_iso), img, B, n_iso)
    assert (want["E"] > 0).mean() >= 0.25                             # the comparison of qa, qb and E means something
    with fic_amd.Encoder(w, w, B, None, n_iso) as enc:
        enc.set_option("search", "lsq")
        enc.set_gray(img)
        for sweep, chunks in ((2, 0), (2, 1), (1, 0)):
            enc.set_option("sweep", sweep)
            enc.set_option("chunks", chunks)
            enc.encode()
            assert enc.last_kernel() == (GENERIC if sweep == 1 else FAST)
            assert_same(results(enc), want, f"sweep {sweep}, chunks {chunks}")
