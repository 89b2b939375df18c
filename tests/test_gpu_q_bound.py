"""The prune bound of k_sweep_q on the device.

  1. The operands the prep kernels store ARE the model's (tests/qmodel.py), bit for bit, through every prep path: the fused
     small launch k_prep_q8<0/2>, k_pool_q<4/8/16>, k_range_q8<0/2>, k_range_q staged and unstaged, 8 isometries as 8 plain
     columns (B = 4) and folded, both MFMA fragment layouts, several planes, a ragged image, flat and letterboxed blocks.  So
     the CPU checks of the bound and its lemmas (tests/test_q_bound.py) speak about the real operands.
  2. Option "q_eshift" (E_r times 2^-k): at k = 0 the stored E_r is the model's exactly; wider thresholds (k < 0, up to every
     pair flagged) give the same codebooks; a threshold 8 times too narrow (k = 3) is CAUGHT on the tight inputs
     (qmodel.tight_image) for every grey mode and block size, against the VALU sweep -- which random images do not do.
     (Joint RGB, k_sweep_q<NK, 3>: tests/test_gpu_rgb_q_bound.py.)"""
import numpy as np
import pytest

import fic_amd
import qmodel as M
from fic_amd import synth
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

KEYS_I = ("idx_local", "idx_global", "iso", "qrows")
KEYS_F = ("a", "b", "err")


def _letterbox(w, h, seed, bar):
    g = synth.image_u(w, h, seed).copy()
    g[:bar] = 16
    g[-bar:] = 16
    g[:, :bar // 2] = 200
    return g


def _check_operands(enc, imgs, B, n_iso, shape16):
    P = len(imgs)
    H, W = imgs[0].shape
    G = M.Geom(W, H, B, n_iso)
    folded = G.mode == 2
    NK = G.NK
    pool_raw = enc.debug_q("pool")
    ntal = pool_raw.size // (P * NK * 64 * 16)
    A_dev = M.decode_frags(pool_raw.reshape(P, -1), G.n, 0 if folded else shape16)
    flat_dev = enc.debug_q("flat").view(np.uint32).reshape(P, ntal)
    rng_raw = enc.debug_q("rng")
    B_dev = M.decode_frags(rng_raw.reshape(P, -1), G.n, 0 if folded else shape16)
    E_dev = enc.debug_q("E").view(np.float32).reshape(P, -1)
    st_dev = enc.debug_q("rng_st").view(np.int32).reshape(P, -1, 2)
    rngC = enc.debug_q("rngC").reshape(P, E_dev.shape[1], G.cpr, G.n)
    dp = enc.debug_pool()
    for p, g in enumerate(imgs):
        pix = M.pool_pixels(g, B)
        assert (dp["pix"][p] == pix).all()
        A = M.domain_operands(pix, B, folded)
        assert (A_dev[p, :G.Nd].view(np.uint16) == A.view(np.uint16)).all(), "domain operands"
        assert (A_dev[p, G.Nd:].view(np.uint16) == 0).all(), "padding rows of the domain store"
        assert (flat_dev[p] == M.dflat(pix, B, G.Nd, ntal)).all(), "flat-tile flags"
        rp = M.range_pixels(g, B)
        rs = M.range_stats(rp, B)
        cols = M.range_columns(rp, B, n_iso).astype(np.float16)
        nc = G.Nr * G.cpr
        assert (B_dev[p, :nc].view(np.uint16) == cols.view(np.uint16)).all(), "range operands"
        assert (B_dev[p, nc:].view(np.uint16) == 0).all(), "padding columns of the range store"
        # E_r: one of the three candidates of the model (the hardware square root is within 1 ulp of the rounded one)
        cand = M.error_bound_candidates(rs["ss"]).view(np.uint32)
        e = E_dev[p, :G.Nr].view(np.uint32)
        assert ((e == cand[0]) | (e == cand[1]) | (e == cand[2])).all(), "E_r"
        assert (E_dev[p, G.Nr:] == M.error_bound(0)).all(), "E_r of the padding ranges (ss = 0)"
        assert (st_dev[p, :G.Nr, 0] == rs["rM"]).all() and (st_dev[p, :G.Nr, 1] == rs["rem"]).all()
        assert (st_dev[p, G.Nr:] == 0).all()
        if G.mode == 0:
            want = rp[:, None, :]
        elif G.mode == 1:
            want = M.copies(rp, B)
        else:
            want = M.copies(rp, B)[:, list(M.PAIR_FIRST)]
        assert (rngC[p, :G.Nr] == want).all(), "byte copies of the exact path"


# (B, n_iso, w, h, planes, q_shape, image kind, the prep kernels the case goes through)
PREP_CASES = [
    (8, 1, 256, 256, 1, 2, "U", "k_prep_q8<0>, 32x32x16 layout"),
    (8, 1, 256, 256, 2, 1, "letterbox", "k_prep_q8<0>, 16x16x32 layout, two planes"),
    (8, 8, 256, 256, 2, 0, "S", "k_prep_q8<2>, two planes"),
    (8, 1, 512, 512, 2, 2, "U", "k_pool_q<8> + k_range_q8<0>"),
    (8, 1, 512, 512, 2, 1, "letterbox", "k_pool_q<8> + k_range_q8<0>, 16x16x32 layout"),
    (8, 8, 512, 512, 2, 0, "letterbox", "k_pool_q<8> + k_range_q8<2>"),
    (4, 1, 200, 200, 1, 0, "U", "k_pool_q<4> + k_range_q staged, ragged"),
    (4, 8, 200, 200, 3, 0, "letterbox", "k_pool_q<4> + k_range_q staged, mode 1, three planes"),
    (16, 1, 256, 256, 1, 1, "S", "k_pool_q<16> + k_range_q staged, 16x16x32 layout"),
    (16, 1, 256, 256, 2, 2, "letterbox", "k_pool_q<16> + k_range_q staged, 32x32x16 layout"),
    (16, 8, 256, 256, 2, 0, "U", "k_pool_q<16> + k_range_q unstaged, folded"),
]


def _image(kind, w, h, seed):
    if kind == "U":
        return synth.image_u(w, h, seed)
    if kind == "S":
        return synth.image_s(w, h, seed)
    return _letterbox(w, h, seed, h // 5)


@pytest.mark.parametrize("B,n_iso,w,h,planes,shape,kind,path", PREP_CASES, ids=[c[-1] for c in PREP_CASES])
def test_device_operands_are_the_model(B, n_iso, w, h, planes, shape, kind, path):
    imgs = [_image(kind, w, h, 300 + 11 * p + B) for p in range(planes)]
    if kind == "letterbox":
        imgs[-1] = np.full((h, w), 93, np.uint8)             # an all-flat plane: every block w = 0, every tile dflat
    with fic_amd.Encoder(w, h, B, None, n_iso, planes) as enc:
        enc.set_option("sweep", 6)
        enc.set_option("q_shape", shape)
        enc.set_gray(np.stack(imgs))
        enc.encode()
        kname = enc.last_kernel()
        fused = kname.endswith("after k_prep_q8, finalising")
        assert fused == path.startswith("k_prep_q8"), kname
        shape16 = 1 if kname.startswith(("k_sweep_q16", )) else 0
        assert shape16 == (1 if shape == 1 else 0), kname
        _check_operands(enc, imgs, B, n_iso, shape16)
        # q_eshift scales the stored E_r by an exact power of two and nothing else
        E0 = enc.debug_q("E").view(np.float32).copy()
        for k in (3, -12):
            enc.set_option("q_eshift", k)
            enc.encode()
            Ek = enc.debug_q("E").view(np.float32)
            assert (Ek.view(np.uint32) == (E0 * np.float32(2.0 ** -k)).view(np.uint32)).all(), k
        enc.set_option("q_eshift", 0)
        enc.encode()
        assert (enc.debug_q("E").view(np.uint32) == E0.view(np.uint32)).all()


def test_q_eshift_is_range_checked():
    with fic_amd.Encoder(64, 64, 4, None, 1) as enc:
        for bad in (-13, 5):
            with pytest.raises(fic_amd.FicError):
                enc.set_option("q_eshift", bad)
    with fic_amd.capi.RgbEncoder(64, 64, 4, 29) as enc:
        for bad in (-13, 5):
            with pytest.raises(fic_amd.FicError):
                enc.set_option("q_eshift", bad)


# ---------------------------------------------------------------------------------------------------------------------
# the sweep on the tight inputs
# ---------------------------------------------------------------------------------------------------------------------
_TIGHT = {}
_VALU = {}


def _tight(B, n_iso, size=None):
    if (B, n_iso, size) not in _TIGHT:
        _TIGHT[(B, n_iso, size)] = M.tight_image(B, n_iso, size=size)[0]
    return _TIGHT[(B, n_iso, size)]


def _valu(name, g, B, n_iso, planes=1):
    """Reference codebook: the VALU sweep (sweep = 2), pinned to the oracle by tests/test_gpu_parity.py."""
    key = (name, B, n_iso, planes)
    if key not in _VALU:
        h, w = g.shape
        with fic_amd.Encoder(w, h, B, None, n_iso, planes) as enc:
            enc.set_option("sweep", 2)
            enc.set_gray(np.stack([g] * planes))
            enc.encode()
            _VALU[key] = {k: v.copy() for k, v in enc.results().items()}
    return _VALU[key]


def _run_q(g, B, n_iso, planes=1, chunks=0, shape=0, eshift=0, stats=False):
    h, w = g.shape
    with fic_amd.Encoder(w, h, B, None, n_iso, planes) as enc:
        enc.set_option("sweep", 6)
        enc.set_option("chunks", chunks)
        enc.set_option("q_shape", shape)
        enc.set_option("q_eshift", eshift)
        if stats:
            enc.set_option("sweep_stats", 1)
        enc.set_gray(np.stack([g] * planes))
        enc.encode()
        r = {k: v.copy() for k, v in enc.results().items()}
        return r, enc.last_kernel(), (enc.sweep_stats() if stats else None), enc.n_ranges


def _mismatches(got, want):
    bad = np.zeros(got["idx_local"].shape, bool)
    for k in KEYS_I:
        d = got[k] != want[k]
        bad |= d.reshape(d.shape[0], d.shape[1], -1).any(2) if d.ndim == 3 else d
    for k in KEYS_F:
        x, y = got[k].view(np.uint32), want[k].view(np.uint32)
        bad |= (x != y) & ~(np.isnan(got[k]) & np.isnan(want[k]))
    return int(bad.sum())


# (B, n_iso) -> runs: (chunks, q_shape, planes, expected kernel name prefix)
def _instantiations(B, n_iso):
    NK, mode = B * B // 16, (0 if n_iso == 1 else (1 if B == 4 else 2))
    # (two chunks of a 117-tile pool are long chunks -- more than FIC_Q_GFAST_TILES = 48 tiles; the 384x384 B = 16, 8-isometry
    #  image has a 64-tile pool, so its long chunks run on the same construction at 512x512)
    runs = [(1, 2, 1, f"k_sweep_q<{NK}, {mode}, false>", None), (10000, 2, 1, f"k_sweep_qs<{NK}, {mode}>", None),
            (2, 2, 1, f"k_sweep_q<{NK}, {mode}, true>", 512 if (B, n_iso) == (16, 8) else None)]
    if mode == 0 and B >= 8:
        runs += [(1, 1, 1, f"k_sweep_q16<{NK}, false>", None), (2, 1, 1, f"k_sweep_q16<{NK}, true>", None),
                 (10000, 1, 1, f"k_sweep_q16s<{NK}>", None)]
    if B == 8:                                                # 8 planes: not a small launch -- k_prep split, separate k_finalize
        runs += [(1, 2, 8, f"k_sweep_q<{NK}, {mode}, false>", None)]
    return runs


# Floors of the flagged-tile path on the tight inputs, one pool chunk: exactly evaluated pairs per range block and the share of
# tile epilogues with flagged pairs.  Measured on the MI355X (exact pairs per range 54 / 246 / 60 / 124 / 583 / 58, flagged
# tiles 0.15-0.44), set at about 60 %.  A random U image of the same size evaluates ~7 pairs per range: the probes' near-ties
# are what drives the exact queue here (its flagged-tile share is not lower -- the pairs, not the tiles, tell them apart).
FLAGGED_FLOOR = {(4, 1): (30, 0.1), (4, 8): (150, 0.1), (8, 1): (35, 0.1), (8, 8): (75, 0.1), (16, 1): (350, 0.1), (16, 8): (35, 0.1)}


@pytest.mark.parametrize("B,n_iso", sorted(M.TIGHT_SHAPES))
def test_every_instantiation_is_exact_on_the_tight_inputs(B, n_iso, capsys):
    """One pool chunk, long chunks, short chunks, both MFMA shapes, the fused small launch (B = 8, one plane) and the separate
    k_finalize (8 planes) -- all bit-identical to the VALU sweep on inputs that sit against the bound; and the flagged-tile
    path was taken: with one pool chunk, exactly evaluated pairs per range block and the share of flagged tile epilogues are
    at least FLAGGED_FLOOR; the exact pairs per range far above what a random image of the same size gives (recorded)."""
    g = _tight(B, n_iso)
    for chunks, shape, planes, name, size in _instantiations(B, n_iso):
        gi = g if size is None else _tight(B, n_iso, size)
        want = _valu(f"tight{size}", gi, B, n_iso, planes)
        got, kname, st, nr = _run_q(gi, B, n_iso, planes, chunks, shape, stats=True)
        if chunks == 1 and planes == 1 and shape == 2:
            per_range, share = st["exact_pairs"] / nr, st["flagged_tiles"] / st["tiles"]
            rnd = _run_q(synth.image_u(g.shape[1], g.shape[0], 23), B, n_iso, 1, 1, 2, stats=True)[2]
            with capsys.disabled():
                print(f"\n[flagged] B={B} n_iso={n_iso}: tight exact pairs / range {per_range:.1f}, flagged tiles {share:.4f}; random U "
                      f"{rnd['exact_pairs'] / nr:.1f}, {rnd['flagged_tiles'] / rnd['tiles']:.4f}")
            fp, fs = FLAGGED_FLOOR[(B, n_iso)]
            assert per_range >= fp and share >= fs, (kname, per_range, share)
        assert kname.startswith(name), (kname, name)
        if B == 8 and planes == 1:
            assert kname.endswith(" after k_prep_q8, finalising"), kname
        if planes > 1:
            assert not kname.endswith("finalising"), kname
        assert _mismatches(got, want) == 0, (kname, chunks)
        # every range evaluates candidate 0 and the probes' near-ties; a flagged tile per 64 tile epilogues at least
        assert st["exact_pairs"] >= 2 * nr * planes, (kname, st)
        assert st["flagged_tiles"] * 64 >= st["tiles"], (kname, st)


@pytest.mark.parametrize("B,n_iso", sorted(M.TIGHT_SHAPES))
def test_wider_threshold_gives_the_same_codebooks(B, n_iso):
    """E_r times 4, 64, 4096 (q_eshift -2 / -6 / -12): more pairs flagged -- at -12 every pair, so the whole pool goes through
    the exact-evaluation queue (FIC_Q_QFLUSH / FIC_Q_QCAP at full load) -- and the same codebooks, on the tight input and on
    two existing images."""
    imgs = {"tight": _tight(B, n_iso), "lena256": np.load(f"{GOLDEN}/lena_grey_256.npy"),
            "S128": synth.image_s(128, 128, synth.SEEDS["cfg2"])}
    for name, g in imgs.items():
        want = _valu(name, g, B, n_iso)
        pairs = []
        for k in (0, -2, -6, -12):
            got, kname, st, nr = _run_q(g, B, n_iso, 1, 1, 0, k, stats=True)
            assert _mismatches(got, want) == 0, (name, k, kname)
            pairs.append(st["exact_pairs"])
        assert pairs[0] <= pairs[1] <= pairs[2] <= pairs[3], (name, pairs)
        # at -12 every pair of every range with rem != 0 is queued (an entry per domain block and sweep column), except in
        # all-flat domain tiles after a chunk's first (every test value 0: nothing to evaluate, slow_tile returns early)
        G = M.Geom(g.shape[1], g.shape[0], B, n_iso)
        live = int((M.range_stats(M.range_pixels(g, B), B)["rem"] != 0).sum())
        nt = (G.Nd + 31) // 32
        flat = M.dflat(M.pool_pixels(g, B), B, G.Nd, nt)
        rows = G.Nd - 32 * int(flat[1:].sum())
        assert pairs[3] >= rows * G.cpr * live, (name, pairs, rows, live)


# smallest shrink caught (from the measured witnesses, tests/test_q_bound.py WITNESS_FLOOR): s = 1/4 (q_eshift 2) where the
# model finds witnesses at 1/4, else 1/8
CAUGHT_AT_2 = {(4, 1), (4, 8), (8, 1), (8, 8), (16, 1)}


@pytest.mark.parametrize("B,n_iso", sorted(M.TIGHT_SHAPES))
def test_too_narrow_threshold_is_caught(B, n_iso, capsys):
    """E_r / 8 (q_eshift = 3) gives at least one codebook entry that differs from the VALU sweep on the tight input, one pool
    chunk, in every grey mode and block size; E_r / 4 (q_eshift = 2) too where the model predicts witnesses at s = 1/4 (all
    but B = 16 with 8 isometries).  Recorded, not asserted: whether random U / S images notice the same shrinks."""
    g = _tight(B, n_iso)
    want = _valu("tight", g, B, n_iso)
    got, kname, _, _ = _run_q(g, B, n_iso, 1, 1, 2, 3)
    bad3 = _mismatches(got, want)
    assert bad3 > 0, f"{kname}: E_r / 8 not caught"
    got, _, _, _ = _run_q(g, B, n_iso, 1, 1, 2, 2)
    bad2 = _mismatches(got, want)
    if (B, n_iso) in CAUGHT_AT_2:
        assert bad2 > 0, f"{kname}: E_r / 4 not caught"
    rnd = {}
    for name, img in (("U", synth.image_u(256, 256, 21)), ("S", synth.image_s(256, 256, 22))):
        ref = _valu(name, img, B, n_iso)
        rnd[name] = {k: _mismatches(_run_q(img, B, n_iso, 1, 1, 2, k)[0], ref) for k in (2, 3, 4)}
    with capsys.disabled():
        print(f"\n[q_eshift] B={B} n_iso={n_iso}: tight input mismatches at E_r/4 {bad2}, E_r/8 {bad3}; random images "
              f"(mismatches at E_r/4, /8, /16): {rnd}")


def test_rgb_wider_threshold_gives_the_same_codebooks():
    """Joint RGB through the matrix-core sweep (k_sweep_q<NK, 3>): E_r (with its Amax factor) times 4 and 4096 gives the same
    codebook as E_r on a natural image.  That a narrower E_r is caught is asserted on the tight colour inputs
    (tests/test_gpu_rgb_q_bound.py); a natural image does not sit against the bound."""
    rgb = np.load(f"{GOLDEN}/lena_colored_256.npy")
    from oracle import fic_oracle as fo
    argb = fo.rgb_to_argb(rgb)
    h, w = rgb.shape[:2]
    for B in (8, 16):
        Dw = fic_amd.geometry(w, h, B)[2]
        res = {}
        for k in (0, -2, -12):
            with fic_amd.capi.RgbEncoder(w, h, B, Dw) as enc:
                enc.set_option("sweep", 2)
                enc.set_option("q_eshift", k)
                enc.set_argb(argb)
                enc.encode()
                assert enc.last_sweep() == 2
                res[k] = enc.results()
        for k in (-2, -12):
            for key in ("idx_local", "qrows"):
                assert (res[k][key] == res[0][key]).all(), (B, k, key)
            for key in ("a", "bR", "bG", "bB"):
                x, y = res[k][key], res[0][key]
                assert ((x.view(np.uint32) == y.view(np.uint32)) | (np.isnan(x) & np.isnan(y))).all(), (B, k, key)


@pytest.mark.parametrize("B", [4, 8, 16])
def test_rgb_device_operands_are_the_model(B):
    """k_pool_qrgb / k_range_qrgb: A = f16(greyD / vD), the B fragments f16(greyR), varianzRange, Amax (the largest rounded-up
    domain norm) and E_r with its Amax factor, against tests/qmodel.py -- bit for bit, the square roots within one ulp as in
    the grey test (E_r is then computed from the device's Amax).  A colour image with flat and low-contrast regions."""
    rng = np.random.default_rng(40 + B)
    S = 128
    rgb = rng.integers(0, 256, (S, S, 3)).astype(np.uint8)
    rgb[:S // 4] = (30, 60, 90)                                     # flat: vD = 0 rows, dflat tiles
    rgb[S // 2:] = (120 + rng.integers(-2, 3, (S // 2, S, 3))).astype(np.uint8)   # small vD: large operands
    from oracle import fic_oracle as fo
    G = M.Geom(S, S, B)
    with fic_amd.capi.RgbEncoder(S, S, B, G.Dw) as enc:
        enc.set_option("sweep", 2)
        enc.set_argb(fo.rgb_to_argb(rgb))
        enc.encode()
        assert enc.last_sweep() == 2
        raw = {k: enc.debug_q(k) for k in enc.Q_STORES}
    psum, msum, vD = M.rgb_pool(rgb, B)
    gR, vR = M.rgb_range(rgb, B)
    A, _ = M.rgb_domain_operands(psum, msum, vD)
    A_dev = M.decode_frags(raw["pool"], G.n, 0)
    assert (A_dev[:G.Nd].view(np.uint16) == A.view(np.uint16)).all(), "domain operands"
    assert (A_dev[G.Nd:].view(np.uint16) == 0).all()
    B_dev = M.decode_frags(raw["rng"], G.n, 0)
    assert (B_dev[:G.Nr].view(np.uint16) == gR.astype(np.float16).view(np.uint16)).all(), "range operands"
    assert (B_dev[G.Nr:].view(np.uint16) == 0).all()
    st = raw["rng_st"].view(np.int32).reshape(-1, 2)
    assert (st[:, 0] == 0).all() and (st[:, 1] == vR).all()
    am = raw["amax"].view(np.float32)[0]
    norms = [M.rgb_domain_operands(psum, msum, vD, u)[1] for u in (-1, 0, 1)]
    assert am in {float(n.max()) for n in norms}, am
    ntal = raw["flat"].size // 4
    flat = np.ones(ntal * 32, bool)
    flat[:G.Nd] = norms[1] == 0
    assert (raw["flat"].view(np.uint32) == flat.reshape(ntal, 32).all(1)).all(), "flat-tile flags"
    E = raw["E"].view(np.uint32)
    cand = [M.rgb_error_bound(gR, am, 0, u).view(np.uint32) for u in (-1, 0, 1)]
    assert ((E == cand[0]) | (E == cand[1]) | (E == cand[2])).all(), "E_r"
