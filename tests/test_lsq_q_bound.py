"""The prune bound of the matrix-core least-squares sweep (k_sweep_lsq_q, fic_lsq_q.hip) on the CPU, from
the numpy restatement tests/lsqqmodel.py: the rounding allowance Er covers the f16 operand error plus the MFMA's accumulation
term on random, extreme and structured blocks (also if f16 subnormals were flushed); theta + Er stays below sqrt(T / n) in exact
arithmetic over the domain of the float chain; an exact hit is final; the model sweep -- theta raised per domain tile, after
the tile's flagged pairs -- gives the codebook of tests/lsqmodel.py; and the multi-level tight images of tests/lsqqtight.py are
what they claim, with the tables the GPU test imports (ER_SHARE, ESHIFT_CAUGHT) derived here from the model alone.  No GPU."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lsqmodel as glm  # noqa: E402
import lsqqmodel as qm  # noqa: E402
import lsqqtight as qt  # noqa: E402
import lsqtight as lt  # noqa: E402
import qmodel  # noqa: E402
import qtmodel  # noqa: E402

CASES = [(B, n_iso) for B in (4, 8, 16) for n_iso in (1, 8)]
IDS = [f"B{B}-iso{n_iso}" for B, n_iso in CASES]


def sample_blocks(B, rng):
    """int64 [*, n]: random blocks (full range, narrow bands, few levels), the extremes -- flat (V = 0), one pixel one level off a
    flat block (the smallest V > 0: n - 1), 0 / 255 in equal halves (the largest V, n^2 255^2 / 4), 0 / 255 with one pixel next to
    the mean (the smallest non-zero |x_i|: subnormal in f16 from B = 8) -- and structured ones (ramps, checkerboards, a spike)."""
    n = B * B
    out = [rng.randint(0, 256, size=(40, n)), rng.randint(100, 110, size=(10, n)), rng.choice([0, 3, 250, 255], size=(20, n)),
           rng.choice([0, 255], size=(10, n))]
    flat = np.full((3, n), 0)
    flat[1], flat[2] = 77, 255
    one = np.full((4, n), 0)
    one[0, 0], one[1, n - 1] = 1, 255
    one[2:], one[2, 3], one[3, 5] = 255, 254, 0
    half = np.where(np.arange(n) < n // 2, 0, 255)
    halves = np.stack([half, half[::-1], np.where(np.arange(n) % 2, 255, 0)])
    near = np.stack([half.copy() for _ in range(6)])
    for i, v in enumerate((127, 128, 126, 129, 120, 135)):
        near[i, i] = v
    near2 = near.copy()
    near2[:, n // 2 + 1] = 128
    # n d_0 - S_d = 1, 2, 3, 5: pixel 0 at v, pixel 1 at w = (n - 1) v - 255 n / 2 - that, the others 0 / 255 in halves
    v = -(-(255 * n // 2 + 6) // (n - 1))
    tiny = np.stack([half.copy() for _ in range(4)])
    for i, t in enumerate((1, 2, 3, 5)):
        tiny[i, 0], tiny[i, 1] = v, (n - 1) * v - 255 * n // 2 - t
        assert 0 <= tiny[i, 1] <= 255 and n * tiny[i, 0] - tiny[i].sum() == t
    ramp = np.stack([np.arange(n) * 255 // (n - 1), (np.arange(n) % B) * 255 // (B - 1), (np.arange(n) // B) * 255 // (B - 1)])
    return np.concatenate([np.asarray(x, np.int64) for x in out + [flat, one, halves, near, near2, tiny, ramp]])


@pytest.mark.parametrize("B", [4, 8, 16])
def test_allowance_covers_the_operand_error(B):
    """|acc_model - q| + the accumulation allowance <= Er for every (pool block, range block, isometry) of the sample, acc_model the
    f64 (exact) dot product of the f16 operands, with Er from the root 1 ulp LOW; the same with every f16 subnormal of the A rows
    flushed to zero.  The accumulation allowance is 2^-24 * 17 NK * sum |A||B| (fic_q.hip's header; the operands here have the
    same ranges: |A| <= 1 with 11 significant bits, B integers of 9 bits)."""
    rng = np.random.RandomState(B)
    d = sample_blocks(B, rng)
    r = sample_blocks(B, rng)
    n, NK = B * B, B * B // 16
    S, _, V, _ = qm.pool_stats(d)
    assert V.min() == 0 and V[V > 0].min() == n - 1 and V.max() == n * n * 255 * 255 // 4 and V.max() < 2 ** 31
    A = qm.a_rows(d, B)
    assert (A[V == 0] == 0).all() and np.isfinite(A.astype(np.float64)).all()
    norm = np.sqrt((A.astype(np.float64) ** 2).sum(1))
    assert np.abs(norm[V > 0] - 1.0).max() < 2.0 ** -10          # the exact row has unit 2-norm
    sub = (A != 0) & (np.abs(A.astype(np.float64)) < 2.0 ** -14)
    if B >= 8:
        assert sub.sum() >= 3, "the sample has no f16 subnormal operand"
    else:
        assert not sub.any()                                      # n V <= 2^26 at B = 4: x_i >= 2^-13
    Bc = qm.b_columns(r, B, 8)
    assert np.abs(Bc).max() <= 255 and (Bc.astype(np.float16).astype(np.int64) == Bc).all()
    st = qm.range_stats(r, B)
    Er = np.repeat(st["Er3"][0].astype(np.float64), 8)[None, :]
    assert (st["Er3"][0] <= st["Er3"][1]).all() and (st["Er3"][1] <= st["Er3"][2]).all()
    q = qm.q_exact(d, Bc, B)
    worst = 0.0
    for rows in (A, qm.flushed(A)):
        err = np.abs(qmodel.acc_exact(rows, Bc) - q) + qmodel.allowance(rows, Bc, NK)
        assert (err <= Er).all(), float((err / Er).max())
        worst = max(worst, float((err / Er).max()))
    # centring: the exact q does not depend on m_r, so the integer sums agree with C / sqrt(n V) of the definition
    cp = qm.copies(r, B, 8).reshape(-1, n)
    C = n * (d @ cp.T) - S[:, None] * np.repeat(st["S_r"], 8)[None, :]
    assert (C == (n * d - S[:, None]) @ Bc.T).all()
    print(f"B={B}: largest (|acc - q| + accumulation) / Er = {worst:.3f}, {int(sub.sum())} subnormal operands")
    assert worst > 0.05                                           # the sample does reach into the allowance


@pytest.mark.parametrize("B", [4, 8, 16])
def test_theta_plus_er_stays_below_the_bound(B):
    """theta + Er < sqrt(T / n) = sqrt(Ti) / (100 B) wherever Ti > 0, in exact rationals, for the three candidates of each root:
    Ti log-uniform, uniform, perfect squares and their neighbours, the corners; Er from ss over its whole range."""
    n = B * B
    R_max = n * n * 255 * 255 // 4
    T_max = 10000 * R_max
    rng = np.random.RandomState(40 + B)
    N = 6000

    def spread(top):
        return np.minimum(np.exp(rng.uniform(0, np.log(top), N)).astype(np.int64), top)

    def squares(top):
        m = np.minimum(np.sqrt(spread(top).astype(np.float64)).astype(np.int64) + 1, int(np.sqrt(top)))
        return np.clip(m * m + rng.randint(-1, 2, N), 0, top)

    corners = np.array([0, 1, 2, 3, 4, T_max - 1, T_max], np.int64)
    Ti = np.concatenate([spread(T_max), rng.randint(0, T_max + 1, N, dtype=np.int64), squares(T_max), np.repeat(corners, 40)])
    ss_max = n * 255 * 255
    ss = np.concatenate([spread(ss_max), rng.randint(0, ss_max + 1, N), squares(ss_max), np.tile(np.array([0, 1, ss_max]), 94)[:corners.size * 40]])
    assert Ti.size == ss.size
    checked = 0
    for eu in (-1, 0, 1):
        Er = qm.allowance_er(ss, B, 0, eu)
        for tu in (-1, 0, 1):
            th = qm.theta(Ti, Er, B, 0, tu)
            for t, e, ti in zip(th.tolist(), Er.tolist(), Ti.tolist()):
                s = Fraction(t) + Fraction(e)
                if ti > 0:
                    assert s < 0 or s * s * (10000 * n) < ti, (ti, t, e)
                    assert t >= 0 or s * s * (10000 * n) < ti     # also where a < Er and the difference is negative
                    checked += 1
                else:
                    assert t < 0                                  # Ti = 0: theta = -Er, everything is flagged
    assert checked >= 9 * 3 * N
    # without the safety factor the chain is NOT below the bound everywhere (Er = 0): the factor is needed, the samples can tell
    raw = qm.theta(Ti, np.zeros(Ti.size, np.float32), B, 0, 0, safety=1.0)
    over = sum(1 for t, ti in zip(raw.tolist(), Ti.tolist()) if Fraction(t) ** 2 * (10000 * n) > ti)
    assert over >= 20
    # the widening of "lsq_tau_widen" puts theta + Er above the bound for large Ti
    wide = qm.theta(np.full(4, T_max), np.zeros(4, np.float32), B, 17)
    assert all(Fraction(t) ** 2 * (10000 * n) > T_max for t in wide.tolist())


def test_an_exact_hit_is_final_and_negative_T_flags_everything():
    R = np.array([0, 5000, 10 ** 9, 7])
    Er = np.full(4, 0.5, np.float32)
    assert (qm.theta_update(R, np.zeros(4, np.int64), Er, 8) == qm.NEVER).all()            # E_best = 0: never flagged again
    th = qm.theta_update(R, np.array([1, 10 ** 9, 1, 10 ** 9]), Er, 8)
    assert th[0] == -1.0 and th[1] == -1.0 and th[3] == -1.0 and th[2] > 0                 # T < 0: theta = -1
    # E >= 0 for every pair: nothing can beat an exact hit, and a later candidate loses the tie
    img, _ = lt.tight_gray(4, 8)
    assert lt.pair_sums(img, 4, 8, False)["E"].min() == 0


@pytest.mark.parametrize("B,n_iso", CASES, ids=IDS)
def test_the_model_sweep_gives_the_models_codebook(B, n_iso):
    """The tile-wise sweep with its prune gives lsqmodel.encode's winners on the tight images of both kinds, in one chunk and in
    chunks of two domain tiles, while it evaluates a small share of the pairs; an exact hit ends a range block's search."""
    for img in (lt.tight_gray(B, n_iso)[0], qt.tight_multilevel(B, n_iso)[0]):
        want = glm.encode(img, B, None, n_iso)
        for tpc in (None, 2):
            got = qm.sweep(img, B, n_iso, tiles_per_chunk=tpc)
            assert (got["E"] == want["E"]).all() and (got["idx_local"] == want["idx_local"]).all() and (got["iso"] == want["iso"]).all()
            assert 0 < got["exact"] < got["pairs"]
        assert qm.sweep(img, B, n_iso)["exact"] < 0.2 * got["pairs"]
    flat = np.full((lt.SIDE[B], lt.SIDE[B]), 77, np.uint8)
    got = qm.sweep(flat, B, n_iso)
    assert (got["c"] == 0).all() and (got["E"] == 0).all()
    nr, nd = (lt.SIDE[B] // B) ** 2, got["pairs"] // ((lt.SIDE[B] // B) ** 2 * n_iso)
    assert got["exact"] == nr * min(32, nd) * n_iso               # the first tile only


@pytest.mark.parametrize("B,n_iso", CASES, ids=IDS)
def test_multilevel_probes_are_what_they_claim(B, n_iso):
    img, table = qt.tight_multilevel(B, n_iso)
    W = lt.SIDE[B]
    n = B * B
    assert img.shape == (W, W) and len(table) >= 32 and len({p["j"] for p in table}) == len(table)
    pool = glm._pool(img, B)
    Dw = int(round(np.sqrt(pool.shape[0])))
    want = glm.encode(img, B, None, n_iso)
    for p in table:
        assert p["E"] == 0 and p["zeros"] == 1 and p["C"] * p["C"] == p["R"] * p["V"]
        d2, d1 = pool[p["g2"]], pool[p["g2"] - 4 * Dw]
        assert np.unique(d2).size >= 3 and ((d2 <= 14) | (d2 >= 240)).all() and (d2 % 2 == 0).all()
        assert np.abs(d1 - d2).sum() == 1 and (p["g2"] - 4 * Dw) // 32 < p["g2"] // 32        # one level off, in an earlier domain tile
    j = np.array([p["j"] for p in table])
    assert (want["idx_local"][j] == [p["g2"] for p in table]).all() and (want["iso"][j] == [p["k"] for p in table]).all()
    assert (want["E"][j] == 0).all() and (want["qrows"][j, 1] == [p["qa"] for p in table]).all()
    # the share of Er that |acc - q| reaches on the winners; the two-level blocks of lsqtight reach none of it
    r = qtmodel.blocks(img, B)
    A, Bc, st = qm.a_rows(pool, B), qm.b_columns(r, B, n_iso), qm.range_stats(r, B)
    col = np.array([p["j"] * n_iso + p["k"] for p in table])
    g2 = np.array([p["g2"] for p in table])
    acc, q = qmodel.acc_exact(A, Bc)[g2, col], qm.q_exact(pool, Bc, B)[g2, col]
    share = (np.abs(acc) - np.abs(q)) / st["Er"][j]
    print(f"B={B} n_iso={n_iso}: share of Er, median {np.median(-share):.3f}, range {(-share).min():.3f} .. {(-share).max():.3f}")
    assert (share < 0).all() and np.median(-share) >= qt.ER_SHARE[B]
    img2, table2 = lt.tight_gray(B, n_iso)
    pool2 = glm._pool(img2, B)
    g = np.array([p["g2"] for p in table2 if not p["copy"]])      # (the same-block pairs have one pixel a level up)
    x = qm.a_rows(pool2[g], B).astype(np.float64)
    assert (np.abs(np.abs(x) - 1.0 / B) == 0).all()               # +-1 / sqrt(n): exact in f16


@pytest.mark.parametrize("B,n_iso", CASES, ids=IDS)
def test_eshift_the_probes_catch(B, n_iso):
    """Teeth: Er times 2^-k narrows the bound below the derivation; the smallest k at which the model sweep loses the winner of a
    quarter of the probes is ESHIFT_CAUGHT.  A pair counts as skipped only if it stays skipped with the accumulation allowance
    added to |acc| (bias = 1).  Every row that changes is a probe and gets a larger E; k <= 0 changes nothing."""
    img, table = qt.tight_multilevel(B, n_iso)
    want = glm.encode(img, B, None, n_iso)
    j = np.array([p["j"] for p in table])
    lost = {}
    for k in (-2, 0, 1, 2, 3, 4):
        got = qm.sweep(img, B, n_iso, eshift=k, bias=1.0)
        ch = np.flatnonzero((got["E"] != want["E"]) | (got["idx_local"] != want["idx_local"]) | (got["iso"] != want["iso"]))
        assert np.isin(ch, j).all() and (got["E"][ch] > want["E"][ch]).all()
        lost[k] = ch.size
    print(f"B={B} n_iso={n_iso}: probes that lose their winner at lsq_q_eshift -2, 0, 1..4: {[lost[k] for k in (-2, 0, 1, 2, 3, 4)]} of {len(table)}")
    assert lost[-2] == 0 and lost[0] == 0
    caught = [k for k in (1, 2, 3, 4) if lost[k] * 4 >= len(table)]
    assert caught and caught[0] == qt.ESHIFT_CAUGHT[(B, n_iso)] and caught == list(range(caught[0], 5))


@pytest.mark.parametrize("B,n_iso", CASES, ids=IDS)
def test_widening_the_two_level_probes_catch(B, n_iso):
    """lsqtight's two-level images on this sweep: theta moves per domain tile, so only probes whose near fit lies in an earlier
    tile than the winner feel "lsq_tau_widen" = WIDEN_CAUGHT -- at least one does at every (B, n_iso), and only probes change."""
    img, table = lt.tight_gray(B, n_iso)
    want = glm.encode(img, B, None, n_iso)
    got = qm.sweep(img, B, n_iso, widen=lt.WIDEN_CAUGHT[(False, B, n_iso)], bias=1.0)
    ch = np.flatnonzero((got["E"] != want["E"]) | (got["idx_local"] != want["idx_local"]) | (got["iso"] != want["iso"]))
    print(f"B={B} n_iso={n_iso}: {ch.size} of {len(table)} probes change under the widening")
    assert ch.size >= 1 and np.isin(ch, [p["j"] for p in table]).all() and (got["E"][ch] > want["E"][ch]).all()
