"""The matrix-core joint-RGB least-squares sweep k_sweep_lsq_rgb_q (colour context option "lsq_engine" = 1, fic_lsq_rgb_q.hip,
DESIGN.md section 4.22) on the GPU against the numpy int64 model tests/rgblsqmodel.py, bit for bit: idx_local, iso, qrows5, E and
the bits of a, bR, bG, bB -- at B = 4 / 8 / 16 on one-block, ragged and multi-chunk pools and a ragged column tile, on the images
of tests/test_gpu_rgb_lsq.py; batched planes; the option's handling; the operands of k_lsq_rgb_q_prep against
tests/rgblsqqmodel.py; the tight images of tests/rgblsqqtight.py; that an allowance too narrow ("lsq_q_eshift" > 0) or a bound too
wide ("lsq_tau_widen") is caught by them; the full-range images, where C needs 64 bits at B = 16; the streams, the decoders and
the collage on such a codebook; "time_sweep".  On a library without the option every case fails at set_option("lsq_engine", ...)."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lsqtight as lt  # noqa: E402
import qtrgbmodel as qr  # noqa: E402
import rgbisomodel as rim  # noqa: E402
import rgblsqmodel as lm  # noqa: E402
import rgblsqqmodel as qm  # noqa: E402
import rgblsqqtight as qt  # noqa: E402
import test_gpu_rgb_lsq as base  # noqa: E402  (its images and its cache of model codebooks)

import fic_amd  # noqa: E402
from fic_amd import capi  # noqa: E402
from conftest import same_f32  # noqa: E402
from oracle import fic_oracle as fo  # noqa: E402

pytestmark = pytest.mark.gpu
E_ARGUMENT, E_STATE = -3, -7

# (w, h, B): one-block pools (one ragged domain tile), 841 pool blocks = 27 tiles with the last ragged, 324 range blocks (a ragged
# column tile), 25 and 289 pool blocks at B = 16
GEOMS = [(8, 8, 4), (16, 16, 4), (32, 32, 8), (32, 32, 16), (64, 64, 4), (144, 144, 8), (64, 64, 16), (160, 160, 16)]
IDS = [f"{g[0]}x{g[1]}-B{g[2]}" for g in GEOMS]
TIGHT = [(4, 1), (4, 8), (8, 1), (8, 8), (16, 1), (16, 8)]
TIGHT_IDS = [f"B{b}-iso{k}" for b, k in TIGHT]

assert_same, results, model = base.assert_same, base.results, base.model


def q_chunks(nd, chunks):
    """Pool chunks the sweep makes of "chunks" = chunks: whole domain tiles of 32 blocks, none empty."""
    ndt = (nd + 31) // 32
    tpc = (ndt + min(chunks, ndt) - 1) // min(chunks, ndt)
    return (ndt + tpc - 1) // tpc


def q_encoder(w, h, B, n_iso, planes=1):
    enc = capi.RgbEncoder(w, h, B, fo.geometry(w, h, B)[2], planes=planes, n_iso=n_iso)
    enc.set_option("search", "lsq")
    enc.set_option("lsq_engine", "mfma")                          # fails on a library without the option
    return enc


def n_domains(w, h, B):
    Dw, Dh = fo.geometry(w, h, B)[2:4]
    return Dw * Dh


def rows_that_differ(got, want):
    bad = np.zeros(want["E"].size, bool)
    for f in ("idx_local", "iso", "E"):
        bad |= np.asarray(got[f]) != want[f]
    return np.flatnonzero(bad)


@pytest.mark.parametrize("n_iso", [1, 8])
@pytest.mark.parametrize("w,h,B", GEOMS, ids=IDS)
def test_codebook_is_the_models(w, h, B, n_iso):
    chunk_runs = (0, 1, 3, 5) if (w, B) == (64, 4) else (0, 1)
    nd = n_domains(w, h, B)
    with q_encoder(w, h, B, n_iso) as enc:
        enc.set_option("sweep_stats", 1)
        pairs = enc.n_ranges * nd * n_iso
        for name, rgb in base.images(w, h).items():
            want = model(name, rgb, B, None, n_iso)
            enc.set_argb(fo.rgb_to_argb(rgb))
            for chunks in chunk_runs:
                enc.set_option("chunks", chunks)
                enc.set_option("sweep", 2 if chunks == 3 or (B == 16 and chunks == 1) else 0)     # "sweep" 0 and 2 both mean this sweep
                enc.encode()
                assert enc.last_kernel() == qm.kernel_name(B, n_iso)
                nch = enc.last_lsq_chunks()
                assert nch == q_chunks(nd, chunks) if chunks else 1 <= nch <= (nd + 31) // 32
                st = enc.sweep_stats()
                assert_same(results(enc), want, f"{name}, chunks {chunks}")
                assert 0 < st["flagged_tiles"] <= st["tiles"] and 0 < st["exact_pairs"] <= pairs and st["waves"] > 0
                if name == "constant":
                    # everything ties, candidate 0 wins with E = 0, and the exact hit ends the search: a chunk's first tile only
                    assert (want["idx_local"] == 0).all() and (want["iso"] == 0).all() and (want["E"] == 0).all()
                    assert st["exact_pairs"] <= enc.n_ranges * n_iso * 32 * nch
                    if nd >= 256 and chunks == 1:
                        assert st["exact_pairs"] * 8 < pairs


def test_three_planes():
    for B, n_iso in ((4, 8), (8, 1), (16, 8)):
        w = h = 64
        names = ("random", "lena", "clamp")
        imgs = [base.images(w, h)[k] for k in names]
        want = [model(k, g, B, None, n_iso) for k, g in zip(names, imgs)]
        with q_encoder(w, h, B, n_iso, planes=3) as enc:
            enc.set_argb(np.stack([fo.rgb_to_argb(g) for g in imgs]))
            for chunks in (0, 2):
                enc.set_option("chunks", chunks)
                enc.encode()
                assert enc.last_kernel() == qm.kernel_name(B, n_iso)
                for p in range(3):
                    assert_same(results(enc, p), want[p], f"B={B}, plane {p}, chunks {chunks}")


def test_option_handling(lena_colored):
    rgb = np.ascontiguousarray(lena_colored[96:160, 64:128])
    argb = fo.rgb_to_argb(rgb)
    B, n_iso = 8, 1
    want = model("lena64", rgb, B, None, n_iso)
    fast, generic = base.kernel_name(B, n_iso, True), base.kernel_name(B, n_iso, False)
    oneshot_before = fic_amd.encode_rgb(argb, 64, 64, B, 13, n_iso=n_iso, search="lsq")
    with capi.RgbEncoder(64, 64, B, 13, n_iso=n_iso) as enc:
        enc.set_argb(argb)
        enc.encode()
        ref = {k: v[0] for k, v in enc.results().items()}
        ref_kernel = enc.last_kernel()
        enc.set_option("lsq_engine", 1)                            # before "search": the order does not matter
        enc.encode()                                                # "search" = 0: the reference encode, whatever the engine
        assert enc.last_kernel() == ref_kernel
        again = {k: v[0] for k, v in enc.results().items()}
        for k in ref:
            assert same_f32(again[k], ref[k]) if ref[k].dtype == np.float32 else (again[k] == ref[k]).all()
        enc.set_option("search", "lsq")
        enc.encode()
        assert enc.last_kernel() == qm.kernel_name(B, n_iso)
        assert_same(results(enc), want, "lsq_engine 1")
        for bad in (2, -1, 7):
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
        enc.set_option("sweep", 1)                                  # "sweep" = 1 never sees the option
        enc.encode()
        assert enc.last_kernel() == generic
        assert_same(results(enc), want, "sweep 1 under lsq_engine 1")
        enc.set_option("sweep", 2)
        enc.encode()
        assert enc.last_kernel() == qm.kernel_name(B, n_iso)
        enc.set_option("lsq_engine", "valu")
        enc.encode()
        assert enc.last_kernel() == fast
        assert_same(results(enc), want, "back at lsq_engine 0")
    # the other order: "search" and "sweep" first, refused engine values in between
    with capi.RgbEncoder(64, 64, B, 13, n_iso=n_iso) as enc:
        enc.set_argb(argb)
        enc.set_option("search", 1)
        enc.set_option("sweep", 2)
        with pytest.raises(fic_amd.FicError) as e:
            enc.set_option("lsq_engine", 2)
        assert e.value.code == E_ARGUMENT
        enc.encode()
        assert enc.last_kernel() == fast                            # the refused value left the default
        enc.set_option("lsq_engine", 1)
        enc.encode()
        assert enc.last_kernel() == qm.kernel_name(B, n_iso)
        assert_same(results(enc), want, "sweep 2, then lsq_engine 1")
    # B = 16: "sweep" = 2 is refused with engine 0 and accepted with engine 1
    want16 = model("lena64", rgb, 16, None, 8)
    with capi.RgbEncoder(64, 64, 16, fo.geometry(64, 64, 16)[2], n_iso=8) as enc:
        enc.set_argb(argb)
        enc.set_option("search", 1)
        enc.encode()
        assert enc.last_kernel() == "k_sweep_lsq_rgb_generic"
        enc.set_option("sweep", 2)
        with pytest.raises(fic_amd.FicError) as e:
            enc.encode()
        assert e.value.code == E_ARGUMENT
        enc.set_option("lsq_engine", 1)
        enc.encode()
        assert enc.last_kernel() == qm.kernel_name(16, 8)
        assert_same(results(enc), want16, "B = 16, sweep 2, lsq_engine 1")
        enc.set_option("lsq_engine", 0)
        with pytest.raises(fic_amd.FicError) as e:
            enc.encode()
        assert e.value.code == E_ARGUMENT
    with capi.RgbEncoder(64, 64, B, 3, n_iso=n_iso) as enc:        # a windowed search keeps the generic sweep
        enc.set_argb(argb)
        enc.set_option("search", "lsq")
        enc.set_option("lsq_engine", 1)
        enc.encode()
        assert enc.last_kernel() == generic
        assert_same(results(enc), model("lena64", rgb, B, 3, n_iso), "window")
        enc.set_option("sweep", 2)
        with pytest.raises(fic_amd.FicError) as e:
            enc.encode()
        assert e.value.code == E_ARGUMENT
    oneshot_after = fic_amd.encode_rgb(argb, 64, 64, B, 13, n_iso=n_iso, search="lsq")     # the cached contexts never carry it
    assert_same(oneshot_before, want, "one-shot before")
    assert_same(oneshot_after, want, "one-shot after")
    assert_same(fic_amd.encode_rgb(argb, 64, 64, B, 13, n_iso=n_iso, search="lsq", lsq_engine="mfma"), want, "encode_rgb(lsq_engine='mfma')")
    assert_same(fic_amd.encode_rgb(argb, 64, 64, B, 13, n_iso=n_iso, search="lsq", lsq_engine="valu"), want, "encode_rgb(lsq_engine='valu')")


@pytest.mark.parametrize("B,n_iso", TIGHT, ids=TIGHT_IDS)
def test_operands_are_the_models(B, n_iso):
    W = qt.SIDE[B]
    img = qt.tight_multilevel(B, n_iso)[0]
    n3, NK = 3 * B * B, 3 * B * B // 16
    with q_encoder(W, W, B, n_iso) as enc:
        enc.set_argb(fo.rgb_to_argb(img))
        enc.encode()
        nr = enc.n_ranges
        raw = {k: enc.debug_lsq_q(k) for k in enc.LSQ_Q_STORES}
    nd = n_domains(W, W, B)
    pool, r = lt._pool(img, B, True), lt._blocks(img, B)
    ndt, nct = (nd + 31) // 32, (nr * n_iso + 31) // 32
    assert raw["A"].size == ndt * NK * 64 * 16 and raw["B"].size == nct * NK * 64 * 16
    A = qm.decode_frags(raw["A"], n3, ndt * 32)
    want_A = qm.a_rows(pool, B)
    same = A[:nd].view(np.uint16) == want_A.view(np.uint16)
    # the conversion may keep f16 subnormals (numpy does) or flush them: the allowance covers both, so either is accepted per element
    assert (same | (A[:nd].view(np.uint16) == qm.flushed(want_A).view(np.uint16))).all() and (A[nd:].view(np.uint16) == 0).all()
    Bq = qm.decode_frags(raw["B"], n3, nct * 32)
    assert (Bq[:nr * n_iso].view(np.uint16) == qm.b_columns(r, B, n_iso).astype(np.float16).view(np.uint16)).all()
    assert (Bq[nr * n_iso:].view(np.uint16) == 0).all()
    st = qm.range_stats(r, B)
    Er, R = raw["Er"].view(np.float32), raw["R"].view(np.uint32)
    assert Er.size == R.size >= nr
    assert (R[:nr] == st["R"]).all() and (R[nr:] == 0).all()
    assert (Er[:nr].view(np.uint32)[None, :] == st["Er3"].view(np.uint32)).any(0).all()      # one of the root's candidates
    assert (Er[nr:] == qm.EABS).all()


def _tight_images(kind, B, n_iso):
    make = qt.two_level if kind == "two-level" else qt.tight_multilevel
    return [make(B, n_iso, seed)[0] for seed in (1, 2)]


@pytest.mark.parametrize("B,n_iso", TIGHT, ids=TIGHT_IDS)
def test_tight_codebooks_are_the_models(B, n_iso):
    W = qt.SIDE[B]
    nd = n_domains(W, W, B)
    for kind in ("two-level", "multi-level"):
        imgs = _tight_images(kind, B, n_iso)
        want = [model((kind, seed), g, B, None, n_iso) for seed, g in zip((1, 2), imgs)]
        # a count that cuts the pool between the near fit's domain tile and the winner's: the bound starts afresh before the winner
        table = (qt.two_level if kind == "two-level" else qt.tight_multilevel)(B, n_iso, 1)[1]
        ndt = (nd + 31) // 32
        cut = next(c for c in range(2, ndt + 1)
                   if any((p["g2"] // 32) % ((ndt + c - 1) // c) == 0 and p["g2"] >= 32 for p in table))
        with q_encoder(W, W, B, n_iso, planes=2) as enc:
            enc.set_option("sweep_stats", 1)
            enc.set_argb(np.stack([fo.rgb_to_argb(g) for g in imgs]))
            pairs = 2 * enc.n_ranges * nd * n_iso
            for chunks in (1, 0, cut):
                enc.set_option("chunks", chunks)
                enc.encode()
                assert enc.last_kernel() == qm.kernel_name(B, n_iso)
                if chunks:
                    assert enc.last_lsq_chunks() == q_chunks(nd, chunks)
                st = enc.sweep_stats()
                for plane in range(2):
                    assert_same(results(enc, plane), want[plane], f"{kind}, plane {plane}, chunks {chunks}")
                print(f"\n[lsq_rgb_q prune] {kind} B={B} n_iso={n_iso} chunks {chunks}: {st['exact_pairs']} of {pairs} pairs flagged, "
                      f"{st['flagged_tiles']} of {st['tiles']} tiles")
                one_tile_chunks = enc.last_lsq_chunks() == ndt            # every tile is a chunk's first: all flagged
                assert 0 < st["exact_pairs"] <= pairs and (one_tile_chunks or st["exact_pairs"] < pairs)


@pytest.mark.parametrize("B,n_iso", TIGHT, ids=TIGHT_IDS)
def test_an_allowance_too_narrow_is_caught(B, n_iso):
    """Er times 2^-k: negative k widens the bound (same codebook, at -12 nearly every pair is evaluated); at the k the model derives
    (rgblsqqtight.ESHIFT_CAUGHT, tests/test_rgb_lsq_q_bound.py) probes lose their winner: every row that differs is a probe with E
    not below the model's.  One pool chunk, so that every probe has its near fit ahead of its winner."""
    W = qt.SIDE[B]
    img, table = qt.tight_multilevel(B, n_iso)
    want = model(("multi-level", 1), img, B, None, n_iso)
    probes = [p["j"] for p in table]
    k = qt.ESHIFT_CAUGHT[(B, n_iso)]
    with q_encoder(W, W, B, n_iso) as enc:
        enc.set_option("chunks", 1)
        enc.set_option("sweep_stats", 1)
        enc.set_argb(fo.rgb_to_argb(img))
        pairs = enc.n_ranges * n_domains(W, W, B) * n_iso
        seen = {}
        for shift in (0, -2, -12):
            enc.set_option("lsq_q_eshift", shift)
            enc.encode()
            seen[shift] = enc.sweep_stats()["exact_pairs"]
            assert_same(results(enc), want, f"lsq_q_eshift {shift}")
        # at -12 the allowance exceeds every |q|: all pairs are flagged until a range block has its exact hit (the model's count;
        # the device's f32 accumulation may move a pair or two across theta)
        full = qm.sweep(img, B, n_iso, eshift=-12)["exact"]
        assert seen[0] <= seen[-2] <= seen[-12] and abs(seen[-12] - full) * 100 <= pairs and seen[0] < seen[-12]
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
    """tau times 1 + 2^-WIDEN_CAUGHT on the two-level images, one pool chunk: the second stage's |C| <= li skips winners."""
    W = qt.SIDE[B]
    img, table = qt.two_level(B, n_iso)
    want = model(("two-level", 1), img, B, None, n_iso)
    probes = [p["j"] for p in table]
    with q_encoder(W, W, B, n_iso) as enc:
        enc.set_option("chunks", 1)
        enc.set_argb(fo.rgb_to_argb(img))
        enc.set_option("lsq_tau_widen", qt.WIDEN_CAUGHT[(B, n_iso)])
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
@pytest.mark.parametrize("w,B,equal,perturb", lt.RGB_FULL, ids=[f"{c[0]}-B{c[1]}-{'equal' if c[2] else 'free'}" for c in lt.RGB_FULL])
def test_full_range_images(w, B, equal, perturb, n_iso):
    """Pixels 0 / 255: V = 2^31.57 and C = +-2^31.55 at B = 16, past a signed 32-bit C and li."""
    img = lt.halves_image(w, w, B, 3, lt.HALVES_SEED, equal=equal, perturb=perturb)
    want = model(("halves", equal), img, B, None, n_iso)
    if B == 16 and w == 160:
        s = lt.pair_sums(img, B, 1, True)
        assert np.abs(s["C"]).max() > 2 ** 31 and s["V"].max() > 2 ** 31
    with q_encoder(w, w, B, n_iso) as enc:
        enc.set_argb(fo.rgb_to_argb(img))
        for chunks in (0, 1):
            enc.set_option("chunks", chunks)
            enc.encode()
            assert enc.last_kernel() == qm.kernel_name(B, n_iso)
            assert_same(results(enc), want, f"chunks {chunks}")


def test_streams_decoders_collage_and_sweep_time_lena64(lena_colored):
    B, n_iso, w, h = 4, 8, 64, 64
    rgb = np.ascontiguousarray(lena_colored[96:160, 64:128])
    argb = fo.rgb_to_argb(rgb)
    wK = fo.geometry(w, h, B)[2]
    want = model("lena64", rgb, B, None, n_iso)
    ref = rim.decode(want["qrows"], want["iso"], w, h, B, wK)
    info = np.stack([want["idx_local"].astype(np.float32), want["a"], want["bR"], want["bG"], want["bB"]], axis=1)
    with q_encoder(w, h, B, n_iso) as enc:
        enc.set_argb(argb)
        enc.encode(with_collage=True)                               # "time_sweep" off: nothing is timed
        enc.sync()
        assert enc.sweep_time() == (0.0, 0)
        enc.set_option("time_sweep", 1)
        t0 = time.perf_counter()
        enc.encode(with_collage=True)
        enc.sync()
        host_ms = (time.perf_counter() - t0) * 1e3
        assert enc.last_kernel() == qm.kernel_name(B, n_iso)
        ms, launches = enc.sweep_time()
        assert launches == 1 and 0 < ms < host_ms
        got = results(enc)
        assert_same(got, want, "lena64")
        run = fic_amd.write_run_rgb_iso(got["qrows"], got["iso"], w, h, B, wK)
        out = fic_amd.decode_rgb_iso_run(run)
        unpack = lambda a: qr.channels(a, w, h).astype(np.uint8)  # noqa: E731
        assert (unpack(out[0]) == ref[0]).all() and same_f32(out[1], ref[1]) and int(out[2]) == ref[2]
        ctx_img, ctx_avg, ctx_it = enc.decode()
        assert (unpack(ctx_img[0]) == ref[0]).all() and same_f32(ctx_avg[0], ref[1]) and int(ctx_it[0]) == ref[2]
        assert (got["collage"] == rim.collage(argb, w, h, B, wK, info, want["iso"])).all()
        enc.set_option("lsq_engine", "valu")                        # the VALU twin is timed by the same option
        enc.encode()
        ms, launches = enc.sweep_time()
        assert launches == 1 and ms > 0


@pytest.mark.parametrize("n_iso", [1, 8])
def test_exact_hits_within_a_tile_keep_the_candidate_order(n_iso):
    """rgblsqqtight.tie_image: the probe's exact hits are pool blocks 1, 4, 7, 10 of the first domain tile, and the kernel
    evaluates block 4 (round 0 of the tile) before block 1 (round 1).  The winner is block 1 only if theta moves after the WHOLE
    tile has been evaluated -- an exact hit in the tile under test must not end the search within it.  With chunks of one tile too."""
    img, j = qt.tie_image()
    want = model("tie", img, 4, None, n_iso)
    assert want["idx_local"][j] == 1 and want["iso"][j] == 0 and want["E"][j] == 0
    with q_encoder(32, 32, 4, n_iso) as enc:
        enc.set_argb(fo.rgb_to_argb(img))
        for chunks in (1, 0, 6):
            enc.set_option("chunks", chunks)
            enc.encode()
            assert enc.last_kernel() == qm.kernel_name(4, n_iso)
            assert_same(results(enc), want, f"chunks {chunks}")
