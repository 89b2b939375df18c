"""The prune bound of the joint-RGB matrix-core sweep k_sweep_q<NK, 3> on the device, on the tight colour inputs of
tests/qmodel.py (tight_rgb_image: every block that can set the pool-wide Amax has the same small vD and nearly the same norm, so
the probe ranges sit against E_r; tests/test_q_bound.py measures how closely, on the model).

  1. Every mode-3 instantiation by name -- one pool chunk, long chunks, short chunks (k_sweep_qs) -- is bit-identical to the
     oracle's encodeRGB and to the VALU sweep, and the flagged-tile path with the reference's f32 sequential sums was taken.
  2. An E_r 4 times too narrow ("q_eshift" = 2, the shrink at which the model finds witnesses) is CAUGHT for every block size;
     wider thresholds give the same codebook with more pairs evaluated exactly.
  3. Amax, shared by atomicMax over the whole pool: batches of planes whose Amax differ by orders of magnitude, and a large pool."""
import numpy as np
import pytest

import fic_amd
import qmodel as M
from fic_amd import synth
from conftest import same_f32

pytestmark = pytest.mark.gpu

_TIGHT = {}
_REF = {}


def _tight(B):
    if B not in _TIGHT:
        _TIGHT[B] = M.tight_rgb_image(B)[0]
    return _TIGHT[B]


def _rgb_synth(w, h, seed):
    return np.stack([synth.image_u(w, h, seed), synth.image_u(w, h, seed + 1), synth.image_u(w, h, seed + 2)], axis=-1)


def _oracle_dict(oracle, rgb, B):
    h, w = rgb.shape[:2]
    ref = oracle.encode_rgb(oracle.rgb_to_argb(rgb), w, h, B, fic_amd.geometry(w, h, B)[2])
    return {"idx_local": ref[:, 0].astype(np.int32), "a": ref[:, 1], "bR": ref[:, 2], "bG": ref[:, 3], "bB": ref[:, 4],
            "qrows": oracle.quantise_rgb(ref)}


def _tight_ref(oracle, B):
    if B not in _REF:
        _REF[B] = _oracle_dict(oracle, _tight(B), B)
    return _REF[B]


def _run(oracle, imgs, B, sweep=2, chunks=0, eshift=0, stats=False, stores=()):
    """Encode a batch of colour images; returns (results, kernel name, counters, raw debug stores of the last plane)."""
    h, w = imgs[0].shape[:2]
    with fic_amd.capi.RgbEncoder(w, h, B, fic_amd.geometry(w, h, B)[2], planes=len(imgs)) as enc:
        enc.set_option("sweep", sweep)
        enc.set_option("chunks", chunks)
        enc.set_option("q_eshift", eshift)
        if stats:
            enc.set_option("sweep_stats", 1)
        enc.set_argb(np.stack([oracle.rgb_to_argb(x) for x in imgs]))
        enc.encode()
        assert enc.last_sweep() == sweep
        r = {k: v.copy() for k, v in enc.results().items()}
        return r, enc.last_kernel(), (enc.sweep_stats() if stats else None), {k: enc.debug_q(k) for k in stores}


def _mismatches(got, want, p=0):
    bad = np.zeros(want["idx_local"].shape, bool)
    for k in ("idx_local", "qrows"):
        d = got[k][p] != want[k]
        bad |= d.any(1) if d.ndim == 2 else d
    for k in ("a", "bR", "bG", "bB"):
        x, y = got[k][p], want[k]
        bad |= (x.view(np.uint32) != y.view(np.uint32)) & ~(np.isnan(x) & np.isnan(y))
    return int(bad.sum())


# Floors of the flagged-tile path on the tight colour inputs, one pool chunk: pairs evaluated exactly (with the f32 sequential
# kovarianz) per range block, and the share of tile epilogues with flagged pairs.  Measured on the MI355X: exact pairs per
# range 50.7 / 70.6 / 375.5, flagged tiles 0.129 / 0.127 / 0.349; floors at about 60 %.  A random colour image of the same size
# evaluates 6.0 / 10.1 / 8.8 pairs per range (flagged tiles 0.176 / 0.257 / 0.337): the pairs, not the tiles, tell them apart.
FLAGGED_FLOOR = {4: (30, 0.075), 8: (42, 0.075), 16: (225, 0.2)}


@pytest.mark.parametrize("B", [4, 8, 16])
def test_every_mode3_instantiation_is_exact_on_the_tight_inputs(oracle, B, capsys):
    """k_sweep_q<NK, 3, false> (one pool chunk), k_sweep_q<NK, 3, true> (two chunks of a 117-tile pool: more than
    FIC_Q_GFAST_TILES each) and k_sweep_qs<NK, 3> (a chunk per two tiles), by name, against the oracle's encodeRGB on inputs
    that sit against the colour bound, and against the VALU sweep where it exists (B = 4 / 8); the one-chunk run took the
    flagged-tile path at least FLAGGED_FLOOR often."""
    rgb = _tight(B)
    NK = B * B // 16
    want = _tight_ref(oracle, B)
    valu, vname, _, _ = _run(oracle, [rgb], B, sweep=1)
    assert vname == (f"k_sweep_rgb_fast<{B * B}>" if B <= 8 else "k_sweep_rgb"), vname
    if B <= 8:
        assert _mismatches(valu, want) == 0, vname
    for chunks, name in ((1, f"k_sweep_q<{NK}, 3, false>"), (2, f"k_sweep_q<{NK}, 3, true>"), (100000, f"k_sweep_qs<{NK}, 3>")):
        got, kname, st, _ = _run(oracle, [rgb], B, chunks=chunks, stats=True)
        assert kname == name, (kname, name)
        nr = want["idx_local"].size
        per_range, share = st["exact_pairs"] / nr, st["flagged_tiles"] / st["tiles"]
        if chunks == 1:
            rnd = _run(oracle, [_rgb_synth(rgb.shape[1], rgb.shape[0], 23)], B, chunks=1, stats=True)[2]
            with capsys.disabled():
                print(f"\n[rgb flagged] B={B}: tight exact pairs / range {per_range:.1f}, flagged tiles {share:.4f}; random colour "
                      f"{rnd['exact_pairs'] / nr:.1f}, {rnd['flagged_tiles'] / rnd['tiles']:.4f}")
            fp, fs = FLAGGED_FLOOR[B]
            assert per_range >= fp and share >= fs, (kname, per_range, share)
        assert _mismatches(got, want) == 0, (kname, chunks)
        if B <= 8:
            assert _mismatches(got, {k: v[0] for k, v in valu.items()}) == 0, (kname, chunks)
        assert st["tiles"] > 0 and st["flagged_tiles"] > 0 and st["exact_pairs"] > 0, (kname, st)


@pytest.mark.parametrize("B", [4, 8, 16])
def test_rgb_too_narrow_threshold_is_caught(oracle, B, capsys):
    """E_r / 4 ("q_eshift" = 2: the smallest shrink at which the model finds witnesses, qmodel.TIGHT_RGB_ESHIFT) gives at
    least one codebook entry that differs from the oracle on the tight colour input, one pool chunk, for every block size.
    E_r times 4, 64, 4096 gives the oracle's codebook, with no fewer pairs evaluated exactly at every step."""
    rgb = _tight(B)
    want = _tight_ref(oracle, B)
    k = M.TIGHT_RGB_ESHIFT[B]
    got, kname, _, _ = _run(oracle, [rgb], B, chunks=1, eshift=k)
    bad = _mismatches(got, want)
    more = {j: _mismatches(_run(oracle, [rgb], B, chunks=1, eshift=j)[0], want) for j in range(k + 1, 5)}
    with capsys.disabled():
        print(f"\n[rgb q_eshift] B={B}: tight colour input mismatches at q_eshift {k}: {bad}; narrower still: {more}")
    assert bad > 0, f"{kname}: E_r / {2 ** k} not caught"
    pairs = []
    for j in (0, -2, -6, -12):
        got, kname, st, _ = _run(oracle, [rgb], B, chunks=1, eshift=j, stats=True)
        assert _mismatches(got, want) == 0, (kname, j)
        pairs.append(st["exact_pairs"])
    assert pairs[0] <= pairs[1] <= pairs[2] <= pairs[3], pairs
    assert pairs[3] > pairs[0], pairs


def _check_amax_and_bound(raw, rgb, B):
    """The stored Amax, flat-tile flags and E_r of one plane against the model (square roots within one ulp: three candidates)."""
    G = M.Geom(rgb.shape[1], rgb.shape[0], B)
    psum, msum, vD = M.rgb_pool(rgb, B)
    gR, vR = M.rgb_range(rgb, B)
    am = raw["amax"].view(np.float32)[0]
    norms = [M.rgb_domain_operands(psum, msum, vD, u)[1] for u in (-1, 0, 1)]
    assert am in {float(x.max()) for x in norms}, (am, [float(x.max()) for x in norms])
    ntal = raw["flat"].size // 4
    flat = np.ones(ntal * 32, bool)
    flat[:G.Nd] = vD == 0
    assert (raw["flat"].view(np.uint32) == flat.reshape(ntal, 32).all(1)).all(), "flat-tile flags"
    E = raw["E"].view(np.uint32)
    cand = [M.rgb_error_bound(gR, am, 0, u).view(np.uint32) for u in (-1, 0, 1)]
    assert ((E == cand[0]) | (E == cand[1]) | (E == cand[2])).all(), "E_r"
    st = raw["rng_st"].view(np.int32).reshape(-1, 2)
    assert (st[:, 1] == vR).all()
    return float(am)


def test_rgb_batch_planes_with_very_different_amax(oracle):
    """planes = 3: a saturated plane with a few odd pixels (Amax about 30), a low-contrast one (Amax about 0.2) and an all-flat
    one (no live block: Amax = 0), in three orders and with one and three pool chunks.  Each plane equals its single-image encode and the oracle, and
    the Amax / E_r / flat flags left in the stores are the LAST plane's own -- an Amax carried over from an earlier plane
    (it is a running atomicMax) would be orders of magnitude off."""
    S, B = 128, 8
    rng = np.random.default_rng(77)
    low = (120 + rng.integers(-2, 3, (S, S, 3))).astype(np.uint8)
    sat = np.zeros((S, S, 3), np.uint8)
    sat[::2, :, 0] = 255
    sat[:, ::2, 1] = 255
    sat[S // 2:, :, 2] = 255
    sat[rng.integers(0, S, 300), rng.integers(0, S, 300)] = rng.integers(0, 256, (300, 3))
    flat = np.full((S, S, 3), (10, 200, 30), np.uint8)
    single = {}
    for name, img in (("low", low), ("sat", sat), ("flat", flat)):
        r, kname, _, raw = _run(oracle, [img], B, stores=fic_amd.capi.RgbEncoder.Q_STORES)
        assert kname.startswith("k_sweep_q"), kname
        want = _oracle_dict(oracle, img, B)
        assert _mismatches(r, want) == 0, name
        single[name] = (want, _check_amax_and_bound(raw, img, B))
    assert single["sat"][1] > 100 * single["low"][1] > 0 and single["flat"][1] == 0, {k: v[1] for k, v in single.items()}
    imgs = {"low": low, "sat": sat, "flat": flat}
    for order in (("low", "sat", "flat"), ("flat", "low", "sat"), ("sat", "flat", "low")):
        for chunks in (1, 3):
            r, kname, st, raw = _run(oracle, [imgs[k] for k in order], B, chunks=chunks, stats=True,
                                     stores=fic_amd.capi.RgbEncoder.Q_STORES)
            for p, name in enumerate(order):
                assert _mismatches(r, single[name][0], p) == 0, (order, chunks, name)
            assert _check_amax_and_bound(raw, imgs[order[-1]], B) == single[order[-1]][1], (order, chunks)


def test_rgb_amax_of_a_large_pool(oracle):
    """512x512 at B = 8 (489 domain tiles, 15 625 blocks): the device's Amax -- one atomicMax per domain tile -- and its flat-tile
    flags equal the model's; the single block that sets Amax sits in the last tile of the pool."""
    S, B = 512, 8
    rng = np.random.default_rng(5)
    rgb = rng.integers(0, 256, (S, S, 3)).astype(np.uint8)
    rgb[:S // 4] = (30, 60, 90)                                    # flat tiles
    rgb[S // 2:] = (120 + rng.integers(-2, 3, (S // 2, S, 3))).astype(np.uint8)
    # bottom-right corner: a scaled block of 63 background pixels and one spike -- vD = 1 and the largest norm of the pool
    rgb[S - 2 * B:, S - 2 * B:] = (50, 50, 50)
    rgb[S - 4:S - 2, S - 4:S - 2] = (50 + 2 * 64 + 1, 50 + 64, 50 + 64)
    G = M.Geom(S, S, B)
    psum, msum, vD = M.rgb_pool(rgb, B)
    norm = M.rgb_domain_operands(psum, msum, vD)[1]
    assert int(np.argmax(norm)) == G.Nd - 1 and vD[-1] == 1, (int(np.argmax(norm)), vD[-1])
    assert norm[-1] > 1.2 * np.sort(norm)[-2]
    r, kname, _, raw = _run(oracle, [rgb], B, stores=fic_amd.capi.RgbEncoder.Q_STORES)
    assert kname.startswith("k_sweep_q"), kname
    am = _check_amax_and_bound(raw, rgb, B)
    assert abs(am - float(norm[-1])) <= 1e-5 * am
    v = _run(oracle, [rgb], B, sweep=1)[0]
    assert _mismatches(r, {k: x[0] for k, x in v.items()}) == 0
