"""The prune bound of the fast least-squares sweeps (k_sweep_lsq_fast; k_sweep_lsq_rgb_fast, section 4.20)
on the CPU: the inequality its derivation promises, in exact integers over the whole domain of the float chain (lsqtight.li_model);
the tight images of tests/lsqtight.py are what they claim to be -- planned winners with E = 0 within 2^-18 .. 2^-23 of the bound,
in every register slot, with same-block near fits; the widening of tau that these probes catch, derived from the model alone
(WIDEN_CAUGHT, which the GPU tests then apply to the kernels); and the full-range images reach the magnitudes the kernels'
comments reason about (V and |C| past 2^31 on the RGB route at B = 16).  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lsqmodel as glm  # noqa: E402
import lsqtight as lt  # noqa: E402
import rgblsqmodel as rlm  # noqa: E402

from oracle import fic_oracle as fo  # noqa: E402

CASES = [(rgb, B, n_iso) for rgb in (False, True) for (B, n_iso) in lt.FAST[rgb]]
IDS = [f"{'rgb' if c[0] else 'grey'}-B{c[1]}-iso{c[2]}" for c in CASES]


def tight(rgb, B, n_iso, seed=1):
    return (lt.tight_rgb if rgb else lt.tight_gray)(B, n_iso, seed)


@pytest.mark.parametrize("rgb,B", [(False, 4), (False, 8), (False, 16), (True, 4), (True, 8)])
def test_li_squared_stays_below_T_V(rgb, B):
    """li^2 S < Ti V (Ti = S T; S = 10^4 grey, 10^6 RGB) wherever Ti V > 0, li = 0 where Ti V = 0 (a skip needs C' = 0 there,
    and C'^2 <= T V' = 0 holds), and li < 2^31: 5 x 350 000 pairs in Python integers -- random ones spread over the orders of
    magnitude, perfect squares and their neighbours in Ti, in V and in both, and the corners of the domain."""
    n, S = B * B, lt.SCALE[rgb]
    R_max = (3 if rgb else 1) * n * n * 255 * 255 // 4           # half the pixels 0, half 255: the largest R and V
    T_max, V_max = S * R_max, R_max
    rng = np.random.RandomState(B + (100 if rgb else 0))
    N = 50000

    def spread(top):                                             # log-uniform over 1 .. top
        return np.minimum(np.exp(rng.uniform(0, np.log(top), N)).astype(np.int64), top)

    def squares(top):                                            # m^2 - 1, m^2, m^2 + 1
        m = np.minimum(np.sqrt(spread(top).astype(np.float64)).astype(np.int64) + 1, int(np.sqrt(top)))
        return np.clip(m * m + rng.randint(-1, 2, N), 0, top)

    ct, cv = [0, 1, 2, T_max - 1, T_max], [0, 1, 2, V_max - 1, V_max]          # the corners, among them {0, 1, S R_max} x {1, 2, V_max}
    parts = [(spread(T_max), spread(V_max)), (rng.randint(0, T_max + 1, N, dtype=np.int64), rng.randint(0, V_max + 1, N, dtype=np.int64)),
             (squares(T_max), spread(V_max)), (spread(T_max), squares(V_max)), (squares(T_max), squares(V_max)),
             (np.repeat(ct, 5), np.tile(cv, 5))]
    parts += [(np.full(N // 5, t), spread(V_max)[:N // 5]) for t in ct] + [(spread(T_max)[:N // 5], np.full(N // 5, v)) for v in cv]
    Ti, V = (np.concatenate([np.asarray(q[i], np.int64) for q in parts]) for i in (0, 1))
    assert Ti.size == V.size >= 350000
    li = lt.li_model(Ti, V, 0, rgb)
    assert (li >= 0).all() and li.max() < 2 ** 31
    lhs = li.astype(object) * li.astype(object) * S
    rhs = Ti.astype(object) * V.astype(object)
    pos = rhs > 0
    bad = np.flatnonzero(pos & ~(lhs < rhs))
    assert bad.size == 0, [(int(Ti[i]), int(V[i]), int(li[i])) for i in bad[:5]]
    assert (li[~pos.astype(bool)] == 0).all() and (~pos.astype(bool)).sum() >= 1000
    # the chain without its safety factor is NOT below the bound everywhere: the factor is needed, the samples can tell
    raw = (np.sqrt(Ti.astype(np.float32)) * np.float32(0.001 if rgb else 0.01) * np.sqrt(V.astype(np.float64)).astype(np.float32)).astype(np.int64)
    assert (raw.astype(object) * raw.astype(object) * S > rhs).sum() >= 100


@pytest.mark.parametrize("rgb,B,n_iso", CASES, ids=IDS)
def test_probes_are_what_they_claim(rgb, B, n_iso):
    NR, NC = lt.FAST[rgb][(B, n_iso)]
    for seed in (1, 2):                                           # the GPU tests put both into one context
        img, table = tight(rgb, B, n_iso, seed)
        W = lt.SIDE[B]
        assert img.shape[:2] == (W, W) and fo.geometry(W, W, B)[2] == fo.geometry(W, W, B)[3]
        assert len(table) >= 32 and len({p["j"] for p in table}) == len(table)
        assert {p["slot"] for p in table} == set(range(NR))
        if n_iso == 8:
            assert sum(p["copy"] for p in table) >= 8
        for p in table:
            assert p["E"] == 0 and p["zeros"] == 1                # the planned candidate fits exactly, and it alone
            assert 0 < p["E_best"] <= 2 * lt.SCALE[rgb] and p["Ti"] > 0
            assert 0 < p["gap"] <= lt.gap_bound(rgb, B, p["copy"]), (p["j"], float(p["gap"]))
            assert p["C"] * p["C"] == p["R"] * p["V"]             # an exact affine image: the continuous optimum has no error
        if seed == 1:
            r = rlm.encode(fo.rgb_to_argb(img), W, W, B, None, n_iso) if rgb else glm.encode(img, B, None, n_iso)
            j = np.array([p["j"] for p in table])
            assert (r["idx_local"][j] == [p["g2"] for p in table]).all() and (r["iso"][j] == [p["k"] for p in table]).all()
            assert (r["E"][j] == 0).all()
            assert (r["qrows"][j, 1] == [p["qa"] * (1000 if rgb else 1) for p in table]).all()
        worst = max(p["gap"] for p in table)
        print(f"{'rgb' if rgb else 'grey'} B={B} n_iso={n_iso} seed {seed}: {len(table)} probes, {sum(p['copy'] for p in table)} same-block, "
              f"largest gap 2^{np.log2(float(worst)):.2f}")


def skipped(table, rgb, widen):
    li = lt.li_model([p["Ti"] for p in table], [p["V"] for p in table], widen, rgb)
    return np.array([int(l) >= abs(p["C"]) for l, p in zip(li, table)])


@pytest.mark.parametrize("rgb,B,n_iso", CASES, ids=IDS)
def test_widening_the_probes_catch(rgb, B, n_iso):
    """Teeth: tau times 1 + 2^-k makes li >= |C'| for the winner of a probe -- a wrong skip -- once 2^-k exceeds the safety
    margin 2^-18 plus the probe's gap.  The largest such k for a quarter of the probes is WIDEN_CAUGHT; as derived (k = 0: no
    widening) the model skips no winner."""
    img, table = tight(rgb, B, n_iso)
    assert not skipped(table, rgb, 0).any()
    caught = [k for k in range(8, 25) if skipped(table, rgb, k).sum() * 4 >= len(table)]
    assert caught and caught == list(range(8, caught[-1] + 1))    # monotone: every coarser widening is caught as well
    print(f"{'rgb' if rgb else 'grey'} B={B} n_iso={n_iso}: probes skipped at k = 15..19: {[int(skipped(table, rgb, k).sum()) for k in range(15, 20)]}")
    assert caught[-1] == lt.WIDEN_CAUGHT[(rgb, B, n_iso)]
    assert 16 <= caught[-1] <= 17


def halves(rgb, w, B, equal, perturb):
    return lt.halves_image(w, w, B, 3 if rgb else 1, lt.HALVES_SEED, equal=equal, perturb=perturb)


def test_full_range_images_reach_the_large_integers():
    for w, B, equal, perturb in lt.RGB_FULL:
        img = halves(True, w, B, equal, perturb)
        s = lt.pair_sums(img, B, 8, True)
        V, C = int(s["V"].max()), s["C"]
        print(f"rgb {w}x{w} B={B} equal={equal}: max V 2^{np.log2(V):.2f}, max C 2^{np.log2(C.max()):.2f}, min C -2^{np.log2(-C.min()):.2f}, "
              f"max n S_dd 2^{np.log2(s['n_dd'].max()):.2f}")
        if B == 16:                                               # past the signed 32 bits in V and in C of both signs; n S_dd wraps
            assert V >= 2 ** 31 and V < 2 ** 32
            assert int(C.max()) >= 2 ** 31 and int(C.min()) <= -2 ** 31
            assert int(s["n_dd"].max()) >= 2 ** 32
        if B == 8:
            assert int(np.abs(C).max()) >= 2 ** 26 and int(np.abs(C).max()) < 2 ** 31
        if perturb:
            assert (np.unique(img).size > 2)
    for w, B, perturb in lt.GRAY_FULL:
        img = halves(False, w, B, False, perturb)
        s = lt.pair_sums(img, B, 8, False)
        print(f"grey {w}x{w} B={B}: max V 2^{np.log2(s['V'].max()):.2f}, max |C| 2^{np.log2(np.abs(s['C']).max()):.2f}")
        assert int(s["V"].max()) < 2 ** 31 and int(np.abs(s["C"]).max()) < 2 ** 31
        if B == 16:
            assert int(np.abs(s["C"]).max()) >= 2 ** 29


def test_halves_image_is_binary_in_cells_of_four():
    img = lt.halves_image(160, 160, 16, 3, lt.HALVES_SEED)
    body = img[2:142, 2:158].reshape(35, 4, 39, 4, 3)             # above the two planted blocks
    assert set(np.unique(img)) == {0, 255} and (body == body[:, :1, :, :1]).all()
    assert 0.4 < (img == 255).mean() < 0.6
    eq = lt.halves_image(160, 160, 16, 3, lt.HALVES_SEED, equal=True)
    assert (eq[..., 0] == eq[..., 1]).all() and (eq[..., 0] == eq[..., 2]).all()
    pool0 = lt._pool(eq, 16, True)[0]
    blocks = lt._blocks(eq, 16)
    assert (blocks[-1] == pool0).all() and (blocks[-2] == 255 - pool0).all()
