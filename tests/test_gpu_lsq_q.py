"""The matrix-core least-squares sweep k_sweep_lsq_q (option "lsq_engine" = 1, fic_lsq_q.hip) on the GPU
against the numpy int64 model tests/lsqmodel.py, bit for bit: idx_local, idx_global, iso, qrows, E and the bits of a, b, err --
on the geometries and images of tests/test_gpu_lsq.py with 1 and 8 isometries, several pool chunk counts, planes and range spans
cut inside a column tile; the option's handling; the operands of k_lsq_q_prep against tests/lsqqmodel.py; the tight images of
tests/lsqtight.py and the multi-level ones of tests/lsqqtight.py; that a bound too narrow ("lsq_q_eshift" > 0) or too wide
("lsq_tau_widen") is caught; full-range images; and a stream written from such a codebook, decoded."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import greyisomodel as gm  # noqa: E402
import lsqmodel as lm  # noqa: E402
import lsqqmodel as qm  # noqa: E402
import lsqqtight as qt  # noqa: E402
import lsqtight as lt  # noqa: E402
import qtmodel  # noqa: E402

import fic_amd  # noqa: E402
from fic_amd import capi, synth  # noqa: E402
from conftest import same_f32  # noqa: E402
from oracle import fic_oracle as fo  # noqa: E402

pytestmark = pytest.mark.gpu
E_ARGUMENT = -3
FIELDS = ("idx_local", "idx_global", "iso", "qrows", "E")
FAST, GENERIC = "k_sweep_lsq_fast", "k_sweep_lsq_generic"
KIND_Q = 7

# (w, h, B): one-block pool; 9 blocks; 25 blocks; 841 blocks, a ragged last domain tile; 324 range blocks, ragged column tiles
GEOMS = [(8, 8, 4), (16, 16, 4), (32, 32, 8), (64, 64, 16), (64, 64, 4), (144, 144, 8)]
IDS = [f"{g[0]}x{g[1]}-B{g[2]}" for g in GEOMS]
TIGHT = [(B, n_iso) for B in (4, 8, 16) for n_iso in (1, 8)]
TIGHT_IDS = [f"B{B}-iso{k}" for B, k in TIGHT]

_MODEL = {}


def clamp_image(w, h, seed=3):
    """tests/test_gpu_lsq.py's: range blocks of full contrast over a nearly flat pool, so that 100 C / V lies far outside -100 .. 100."""
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


def model(key, g, B, n_iso):
    key = (key, g.shape, B, n_iso)
    if key not in _MODEL:
        _MODEL[key] = lm.encode(g, B, None, n_iso)
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


def q_chunks(nd, chunks):
    """Pool chunks the sweep makes of "chunks" = chunks: whole domain tiles of 32 blocks, none empty."""
    ndt = (nd + 31) // 32
    tpc = (ndt + min(chunks, ndt) - 1) // min(chunks, ndt)
    return (ndt + tpc - 1) // tpc


def lsq_q_encoder(w, h, B, n_iso, planes=1):
    enc = fic_amd.Encoder(w, h, B, None, n_iso, planes=planes)
    enc.set_option("search", "lsq")
    enc.set_option("lsq_engine", "mfma")
    return enc


def rows_that_differ(got, want):
    bad = np.zeros(want["E"].size, bool)
    for f in ("idx_local", "iso", "E"):
        bad |= np.asarray(got[f]) != want[f]
    return np.flatnonzero(bad)


@pytest.mark.parametrize("n_iso", [1, 8])
@pytest.mark.parametrize("w,h,B", GEOMS, ids=IDS)
def test_codebook_is_the_models(w, h, B, n_iso):
    chunk_runs = (0, 1, 3, 5) if (w, B) == (64, 4) else (0, 1)
    with lsq_q_encoder(w, h, B, n_iso) as enc:
        enc.set_option("sweep_stats", 1)
        nd, pairs = enc.n_domains, enc.n_ranges * enc.n_domains * n_iso
        for name, g in images(w, h).items():
            want = model(name, g, B, n_iso)
            enc.set_gray(g)
            for chunks in chunk_runs:
                enc.set_option("chunks", chunks)
                enc.set_option("sweep", 2 if chunks == 3 else 0)          # "sweep" 0 and 2 both mean this sweep
                enc.encode()
                assert enc.last_kernel() == qm.kernel_name(B, n_iso)
                info = enc.info()
                assert info["sweep_kind"] == KIND_Q
                if chunks:
                    assert info["chunks"] == q_chunks(nd, chunks)
                st = enc.sweep_stats()
                assert_same(results(enc), want, f"{name}, chunks {chunks}")
                assert 0 < st["flagged_tiles"] <= st["tiles"] and 0 < st["exact_pairs"] <= pairs and st["waves"] > 0
                if name == "constant":
                    # everything ties, candidate 0 wins with E = 0, and the exact hit ends the search: a chunk's first tile only
                    assert (want["idx_local"] == 0).all() and (want["iso"] == 0).all() and (want["E"] == 0).all()
                    assert st["exact_pairs"] <= enc.n_ranges * n_iso * 32 * info["chunks"]
                    if nd >= 256 and chunks == 1:
                        assert st["exact_pairs"] * 8 < pairs


def test_three_planes_in_two_spans():
    for B, n_iso in ((4, 8), (8, 1)):
        w = h = 64
        names = ("U", "S", "clamp")
        imgs = [images(w, h)[k] for k in names]
        want = [model(k, g, B, n_iso) for k, g in zip(names, imgs)]
        with lsq_q_encoder(w, h, B, n_iso, planes=3) as enc:
            enc.set_gray(np.stack(imgs))
            nr = enc.n_ranges
            cut = nr // 2 + 5 if n_iso == 1 else nr // 2 + 1        # inside a column tile of 32 columns (32 or 4 range blocks)
            assert (cut * n_iso) % 32 != 0
            for spans in (((0, -1),), ((0, cut), (cut, nr - cut)), ((cut, -1), (0, cut))):
                for b, c in spans:
                    enc.encode(b, c)
                    assert enc.last_kernel() == qm.kernel_name(B, n_iso)
                for p in range(3):
                    assert_same(results(enc, p), want[p], f"B={B}, plane {p}, spans {spans}")
            # results outside a span are untouched: another image, one span, the other rows keep the old codebook
            enc.set_gray(np.stack(imgs[::-1]))
            enc.encode(cut, nr - cut)
            for p in range(3):
                got, old, new = results(enc, p), want[p], want[2 - p]
                for f in FIELDS:
                    assert (np.asarray(got[f])[:cut] == old[f][:cut]).all() and (np.asarray(got[f])[cut:] == new[f][cut:]).all()


def test_option_handling(lena64):
    B, n_iso = 8, 1
    want = model("lena64", lena64, B, n_iso)
    oneshot_before = capi.encode_gray_oneshot(lena64, B, None, n_iso, search="lsq")
    with fic_amd.Encoder(64, 64, B, None, n_iso) as enc:
        enc.set_gray(lena64)
        enc.encode()
        ref = results_ref(enc)
        enc.set_option("lsq_engine", 1)                            # fails on a library without the option
        enc.encode()                                                # "search" = 0: the reference encode, whatever the engine
        assert enc.info()["sweep_kind"] != KIND_Q and not enc.last_kernel().startswith("k_sweep_lsq")
        again = results_ref(enc)
        for k in ref:
            assert same_f32(again[k], ref[k]) if ref[k].dtype == np.float32 else (again[k] == ref[k]).all()
        enc.set_option("search", "lsq")
        enc.encode()
        assert enc.last_kernel() == qm.kernel_name(B, n_iso)
        assert_same(results(enc), want, "lsq_engine 1")
        for bad in (2, -1):
            with pytest.raises(fic_amd.FicError) as e:
                enc.set_option("lsq_engine", bad)
            assert e.value.code == E_ARGUMENT
        with pytest.raises(fic_amd.FicError) as e:
            enc.set_option("lsq_engine", "tensor")
        assert e.value.code == E_ARGUMENT
        for bad in (3, 5, 6, -1):                                   # "sweep" keeps its values under "search" = 1
            with pytest.raises(fic_amd.FicError) as e:
                enc.set_option("sweep", bad)
            assert e.value.code == E_ARGUMENT
        for bad in (5, -13):
            with pytest.raises(fic_amd.FicError) as e:
                enc.set_option("lsq_q_eshift", bad)
            assert e.value.code == E_ARGUMENT
        enc.encode()                                                # the refused values changed nothing
        assert enc.last_kernel() == qm.kernel_name(B, n_iso)
        assert_same(results(enc), want, "after refused values")
        enc.set_option("sweep", 1)
        enc.encode()
        assert enc.last_kernel() == GENERIC and enc.info()["sweep_kind"] == 1
        assert_same(results(enc), want, "sweep 1 under lsq_engine 1")
        enc.set_option("sweep", 0)
        enc.set_option("lsq_engine", "valu")
        enc.encode()
        assert enc.last_kernel() == FAST and enc.info()["sweep_kind"] == 2
        assert_same(results(enc), want, "back at lsq_engine 0")
    with fic_amd.Encoder(64, 64, B, 3, n_iso) as enc:               # a windowed search keeps the generic sweep
        enc.set_gray(lena64)
        enc.set_option("search", "lsq")
        enc.set_option("lsq_engine", 1)
        enc.encode()
        assert enc.last_kernel() == GENERIC
        assert_same(results(enc), lm.encode(lena64, B, 3, n_iso), "window")
        enc.set_option("sweep", 2)
        with pytest.raises(fic_amd.FicError) as e:
            enc.encode()
        assert e.value.code == E_ARGUMENT
    oneshot_after = capi.encode_gray_oneshot(lena64, B, None, n_iso, search="lsq")
    for k in ("idx_local", "iso", "qrows", "E"):
        assert (oneshot_before[k] == oneshot_after[k]).all() and (oneshot_after[k] == want[k]).all()
    assert same_f32(oneshot_before["a"], oneshot_after["a"]) and same_f32(oneshot_before["b"], oneshot_after["b"])
    r = fic_amd.encode_gray(lena64, B, None, n_iso, search="lsq", lsq_engine="mfma")
    assert_same(r, want, "fic_amd.encode_gray(lsq_engine='mfma')")
    assert_same(fic_amd.encode_gray(lena64, B, None, n_iso, search="lsq", lsq_engine="valu"), want, "lsq_engine='valu'")


def results_ref(enc):
    return {k: v[0] for k, v in enc.results().items()}


@pytest.mark.parametrize("B,n_iso", TIGHT, ids=TIGHT_IDS)
def test_operands_are_the_models(B, n_iso):
    W = lt.SIDE[B]
    img = qt.tight_multilevel(B, n_iso)[0]
    n, NK = B * B, B * B // 16
    with lsq_q_encoder(W, W, B, n_iso) as enc:
        enc.set_gray(img)
        enc.encode()
        nd, nr = enc.n_domains, enc.n_ranges
        raw = {k: enc.debug_lsq_q(k) for k in enc.LSQ_Q_STORES}
    pool, r = lm._pool(img, B), qtmodel.blocks(img, B)
    ndt, nct = (nd + 31) // 32, (nr * n_iso + 31) // 32
    assert raw["A"].size == ndt * NK * 64 * 16 and raw["B"].size == nct * NK * 64 * 16
    A = qm.decode_frags(raw["A"], n, ndt * 32)
    assert (A[:nd].view(np.uint16) == qm.a_rows(pool, B).view(np.uint16)).all() and (A[nd:].view(np.uint16) == 0).all()
    Bq = qm.decode_frags(raw["B"], n, nct * 32)
    assert (Bq[:nr * n_iso].view(np.uint16) == qm.b_columns(r, B, n_iso).astype(np.float16).view(np.uint16)).all()
    assert (Bq[nr * n_iso:].view(np.uint16) == 0).all()
    st = qm.range_stats(r, B)
    Er, R = raw["Er"].view(np.float32), raw["R"].view(np.uint32)
    assert Er.size == R.size >= nr
    assert (R[:nr] == st["R"]).all() and (R[nr:] == 0).all()
    assert (Er[:nr].view(np.uint32)[None, :] == st["Er3"].view(np.uint32)).any(0).all()      # one of the root's candidates
    assert (Er[nr:] == qm.EABS).all()


@pytest.mark.parametrize("B,n_iso", TIGHT, ids=TIGHT_IDS)
def test_tight_codebooks_are_the_models(B, n_iso):
    W = lt.SIDE[B]
    cut = lt.cutting_chunks(B, lt.tight_gray(B, n_iso, 1)[1], False)
    for kind, make in (("two-level", lt.tight_gray), ("multi-level", qt.tight_multilevel)):
        imgs = [make(B, n_iso, seed)[0] for seed in (1, 2)]
        want = [model((kind, seed), g, B, n_iso) for seed, g in zip((1, 2), imgs)]
        with lsq_q_encoder(W, W, B, n_iso, planes=2) as enc:
            enc.set_option("sweep_stats", 1)
            enc.set_gray(np.stack(imgs))
            pairs = 2 * enc.n_ranges * enc.n_domains * n_iso
            for chunks in (1, 0, cut):
                enc.set_option("chunks", chunks)
                enc.encode()
                assert enc.last_kernel() == qm.kernel_name(B, n_iso)
                if chunks:
                    assert enc.info()["chunks"] == q_chunks(enc.n_domains, chunks)
                st = enc.sweep_stats()
                for plane in range(2):
                    assert_same(results(enc, plane), want[plane], f"{kind}, plane {plane}, chunks {chunks}")
                print(f"\n[lsq_q prune] {kind} B={B} n_iso={n_iso} chunks {chunks}: {st['exact_pairs']} of {pairs} pairs flagged, "
                      f"{st['flagged_tiles']} of {st['tiles']} tiles")
                one_tile_chunks = enc.info()["chunks"] == (enc.n_domains + 31) // 32      # every tile is a chunk's first: all flagged
                assert 0 < st["exact_pairs"] <= pairs and (one_tile_chunks or st["exact_pairs"] < pairs)


@pytest.mark.parametrize("B,n_iso", TIGHT, ids=TIGHT_IDS)
def test_an_allowance_too_narrow_is_caught(B, n_iso):
    """Er times 2^-k: negative k widens the bound (same codebook, at -12 nearly every pair is evaluated); at the k the model derives
    (lsqqtight.ESHIFT_CAUGHT, tests/test_lsq_q_bound.py) probes lose their winner: every row that differs is a probe with E not
    below the model's.  One pool chunk, so that every probe has its near fit ahead of its winner."""
    W = lt.SIDE[B]
    img, table = qt.tight_multilevel(B, n_iso)
    want = model(("multi-level", 1), img, B, n_iso)
    probes = [p["j"] for p in table]
    k = qt.ESHIFT_CAUGHT[(B, n_iso)]
    with lsq_q_encoder(W, W, B, n_iso) as enc:
        enc.set_option("chunks", 1)
        enc.set_option("sweep_stats", 1)
        enc.set_gray(img)
        pairs = enc.n_ranges * enc.n_domains * n_iso
        seen = {}
        for shift in (0, -2, -12):
            enc.set_option("lsq_q_eshift", shift)
            enc.encode()
            seen[shift] = enc.sweep_stats()["exact_pairs"]
            assert_same(results(enc), want, f"lsq_q_eshift {shift}")
        # at -12 the allowance exceeds every |q|: all pairs are flagged until a range block has its exact hit (the model's count;
        # the device's f32 accumulation may move a pair or two across theta)
        full = qm.sweep(img, B, n_iso, eshift=-12)["exact"]
        assert seen[0] <= seen[-2] <= seen[-12] and abs(seen[-12] - full) * 100 <= pairs and seen[-12] * 2 >= pairs and seen[0] * 4 <= seen[-12]
        enc.set_option("lsq_q_eshift", k)
        enc.encode()
        narrow = results(enc)
        bad = rows_that_differ(narrow, want)
        print(f"\n[lsq_q_eshift] B={B} n_iso={n_iso}: {bad.size} of {len(probes)} probe rows differ at k = {k}; pairs flagged at 0 / -2 / -12: "
              f"{seen[0]} / {seen[-2]} / {seen[-12]} of {pairs}")
        assert bad.size >= 1 and np.isin(bad, probes).all()
        assert (narrow["E"][bad] >= want["E"][bad]).all()
        enc.set_option("lsq_q_eshift", 0)
        enc.encode()
        assert_same(results(enc), want, "lsq_q_eshift back at 0")


@pytest.mark.parametrize("B,n_iso", TIGHT, ids=TIGHT_IDS)
def test_a_bound_too_wide_is_caught(B, n_iso):
    """tau times 1 + 2^-WIDEN_CAUGHT on lsqtight's two-level images, one pool chunk: the second stage's |C| <= li skips winners."""
    W = lt.SIDE[B]
    img, table = lt.tight_gray(B, n_iso)
    want = model(("two-level", 1), img, B, n_iso)
    probes = [p["j"] for p in table]
    with lsq_q_encoder(W, W, B, n_iso) as enc:
        enc.set_option("chunks", 1)
        enc.set_gray(img)
        enc.set_option("lsq_tau_widen", lt.WIDEN_CAUGHT[(False, B, n_iso)])
        enc.encode()
        assert enc.last_kernel() == qm.kernel_name(B, n_iso)
        wide = results(enc)
        bad = rows_that_differ(wide, want)
        print(f"\n[lsq_tau_widen] B={B} n_iso={n_iso}: {bad.size} of {len(probes)} probe rows differ")
        assert bad.size >= 1 and np.isin(bad, probes).all() and (wide["E"][bad] >= want["E"][bad]).all()
        enc.set_option("lsq_tau_widen", 0)
        enc.encode()
        assert_same(results(enc), want, "lsq_tau_widen back at 0")


@pytest.mark.parametrize("n_iso", [1, 8])
@pytest.mark.parametrize("w,B,perturb", lt.GRAY_FULL, ids=[f"{c[0]}-B{c[1]}" for c in lt.GRAY_FULL])
def test_full_range_images(w, B, perturb, n_iso):
    img = lt.halves_image(w, w, B, 1, lt.HALVES_SEED, perturb=perturb)
    want = model("halves", img, B, n_iso)
    with lsq_q_encoder(w, w, B, n_iso) as enc:
        enc.set_gray(img)
        for chunks in (0, 1):
            enc.set_option("chunks", chunks)
            enc.encode()
            assert enc.last_kernel() == qm.kernel_name(B, n_iso)
            assert_same(results(enc), want, f"chunks {chunks}")


def test_streams_decoders_and_collage_lena64(lena64):
    B, n_iso = 4, 8
    h, w = lena64.shape
    wK = fo.geometry(w, h, B)[2]
    want = model("lena64", lena64, B, n_iso)
    ref = fo.decode_rows(want["qrows"], want["iso"], w, h, B, wK)
    with lsq_q_encoder(w, h, B, n_iso) as enc:
        enc.set_option("time_sweep", 1)
        enc.set_gray(lena64)
        enc.encode()
        assert enc.last_kernel() == qm.kernel_name(B, n_iso)
        ms, launches = enc.sweep_time()
        assert launches == 1 and ms > 0
        got = results(enc)
        assert_same(got, want, "lena64")
        run = fic_amd.write_run_gray_iso(got["qrows"], got["iso"], w, h, B, wK)
        img, avg, it = fic_amd.decode_gray_iso_run(run)
        assert (img == ref[0]).all() and avg.view(np.uint32) == ref[1].view(np.uint32) and it == ref[2]
        ctx_img, ctx_avg, ctx_it = enc.decode()
        assert (ctx_img[0] == ref[0]).all() and ctx_avg[0].view(np.uint32) == ref[1].view(np.uint32) and ctx_it[0] == ref[2]
        painted = gm.collage(lena64, B, want["idx_global"], want["a"], want["b"], want["iso"])[0]
        assert (enc.collage()[0] == painted).all()
