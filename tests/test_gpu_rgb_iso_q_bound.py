"""The prune bound of the joint-RGB matrix-core sweep with 8 isometries, k_sweep_q<NK, 4>, on the device, on the tight colour
inputs of tests/qmodel.py (tight_rgb_image: the probe ranges sit against E_r).  The twin of tests/test_gpu_rgb_q_bound.py for the
new mode; E_r depends on a range block's values, not their positions, so MODE 3's bound must hold for each of the 8 columns.

  1. Every mode-4 instantiation by name -- one pool chunk, long chunks, short chunks (k_sweep_qs) -- gives the codebook of the
     VALU sweep (k_sweep_rgb_fast_iso / k_sweep_rgb_iso, which evaluate every (range, domain, isometry) triple), and
     sweep_stats shows flagged tiles and pairs evaluated exactly.
  2. "q_eshift" <= 0 (E_r as derived, or wider) gives the VALU codebook with no fewer pairs evaluated exactly at every step; an
     E_r 4 times too narrow ("q_eshift" = 2, the shrink at which the model finds witnesses for MODE 3) is CAUGHT.
  3. The stores: pool operands, flat flags, Amax, E_r and varianzRange are those of the 1-isometry mode; the range operand has 8
     columns per range block, column k the copy with c_k[src_k(i)] = greyR[i]."""
import numpy as np
import pytest

import fic_amd
import qmodel as M
import rgbisomodel as rm

pytestmark = pytest.mark.gpu

_TIGHT = {}
_VALU = {}


def _tight(B):
    if B not in _TIGHT:
        _TIGHT[B] = M.tight_rgb_image(B)[0]
    return _TIGHT[B]


def _run(oracle, rgb, B, sweep=2, chunks=0, eshift=0, stats=False, stores=(), n_iso=8):
    h, w = rgb.shape[:2]
    with fic_amd.capi.RgbEncoder(w, h, B, fic_amd.geometry(w, h, B)[2], n_iso=n_iso) as enc:
        enc.set_option("sweep", sweep)
        enc.set_option("chunks", chunks)
        enc.set_option("q_eshift", eshift)
        if stats:
            enc.set_option("sweep_stats", 1)
        enc.set_argb(oracle.rgb_to_argb(rgb))
        enc.encode()
        assert enc.last_sweep() == sweep
        r = {k: v[0].copy() for k, v in enc.results().items()}
        return r, enc.last_kernel(), (enc.sweep_stats() if stats else None), {k: enc.debug_q(k) for k in stores}


def _valu(oracle, B):
    if B not in _VALU:
        r, name, _, _ = _run(oracle, _tight(B), B, sweep=1)
        assert name == (f"k_sweep_rgb_fast_iso<{B * B}>" if B <= 8 else "k_sweep_rgb_iso"), name
        _VALU[B] = r
    return _VALU[B]


def _mismatches(got, want):
    bad = np.zeros(want["idx_local"].shape, bool)
    for k in ("idx_local", "iso", "qrows"):
        d = got[k] != want[k]
        bad |= d.any(1) if d.ndim == 2 else d
    for k in ("a", "bR", "bG", "bB"):
        x, y = got[k], want[k]
        bad |= (x.view(np.uint32) != y.view(np.uint32)) & ~(np.isnan(x) & np.isnan(y))
    return int(bad.sum())


@pytest.mark.parametrize("B", [4, 8, 16])
def test_every_mode4_instantiation_is_exact_on_the_tight_inputs(oracle, B, capsys):
    rgb = _tight(B)
    NK = B * B // 16
    want = _valu(oracle, B)
    h, w = rgb.shape[:2]
    rows = np.arange(1, want["idx_local"].size, 37)                   # the VALU reference itself against the model, on a sample
    ref = rm.encode(oracle.rgb_to_argb(rgb), w, h, B, fic_amd.geometry(w, h, B)[2], 8, rows=rows)
    assert (want["idx_local"][rows] == ref["info"][rows, 0].astype(np.int32)).all() and (want["iso"][rows] == ref["iso"][rows]).all()
    assert (want["qrows"][rows] == ref["qrows"][rows]).all()
    for chunks, name in ((1, f"k_sweep_q<{NK}, 4, false>"), (2, f"k_sweep_q<{NK}, 4, true>"), (100000, f"k_sweep_qs<{NK}, 4>")):
        got, kname, st, _ = _run(oracle, rgb, B, chunks=chunks, stats=True)
        assert kname == name, (kname, name)
        if chunks == 1:
            with capsys.disabled():
                print(f"\n[rgb iso flagged] B={B}: exact triples / range {st['exact_pairs'] / want['idx_local'].size:.1f}, "
                      f"flagged tiles {st['flagged_tiles'] / st['tiles']:.4f}")
        assert _mismatches(got, want) == 0, (kname, chunks)
        assert st["tiles"] > 0 and st["flagged_tiles"] > 0 and st["exact_pairs"] > 0, (kname, st)


@pytest.mark.parametrize("B", [4, 8, 16])
def test_rgb_iso_too_narrow_threshold_is_caught(oracle, B, capsys):
    rgb = _tight(B)
    want = _valu(oracle, B)
    k = M.TIGHT_RGB_ESHIFT[B]
    got, kname, _, _ = _run(oracle, rgb, B, chunks=1, eshift=k)
    bad = _mismatches(got, want)
    with capsys.disabled():
        print(f"\n[rgb iso q_eshift] B={B}: tight colour input mismatches at q_eshift {k}: {bad}")
    assert bad > 0, f"{kname}: E_r / {2 ** k} not caught"
    pairs = []
    for j in (0, -2, -6, -12):
        got, kname, st, _ = _run(oracle, rgb, B, chunks=1, eshift=j, stats=True)
        assert _mismatches(got, want) == 0, (kname, j)
        pairs.append(st["exact_pairs"])
    assert pairs[0] <= pairs[1] <= pairs[2] <= pairs[3], pairs
    assert pairs[3] > pairs[0], pairs


@pytest.mark.parametrize("B", [4, 8, 16])
def test_stores_have_eight_permuted_columns_per_range(oracle, B):
    rgb = _tight(B)
    n, NK = B * B, B * B // 16
    stores = fic_amd.capi.RgbEncoder.Q_STORES
    r1 = _run(oracle, rgb, B, chunks=1, stores=stores, n_iso=1)[3]
    r8 = _run(oracle, rgb, B, chunks=1, stores=stores, n_iso=8)[3]
    for k in ("pool", "flat", "E", "rng_st", "amax"):                 # nothing of these depends on the pixel order of a range block
        assert (r1[k] == r8[k]).all(), k
    nr = r8["E"].size // 4

    def columns(raw):                                                 # [columns, n] f16: fragment (ct, m, lane) holds positions 16 m + 8 (lane >> 5) ..+8 of column 32 ct + (lane & 31)
        a = raw.view(np.float16).reshape(-1, NK, 2, 32, 8)
        return a.transpose(0, 3, 1, 2, 4).reshape(-1, n)

    c1, c8 = columns(r1["rng"]), columns(r8["rng"])
    src = rm.iso_table(B)
    for k in range(8):
        ck = c8[k:8 * nr:8]
        assert (ck[:, src[k]] == c1[:nr]).all(), k                    # c_k[src_k(i)] = greyR[i]
    assert (c8[8 * nr:] == 0).all()
