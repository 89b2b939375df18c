"""Tight inputs for the matrix-core least-squares sweep (k_sweep_lsq_q) whose domain blocks have SEVERAL
grey levels.  The images of tests/lsqtight.py have two levels in equal halves, so the normalised operand x_i = +-1 / sqrt(n) is
exact in f16 at every B and |acc - q| is zero: they sit on the bound of 4.19 but do not exercise the f16 allowance Er.  Here
every pixel of a design block d2 is drawn from a few even levels <= 14 or >= 240; otherwise the construction is lsqtight's: d1
is d2 with one pixel one level off and comes earlier in the pool -- here one block row higher, 4 Dw pool blocks and so several
domain tiles earlier, because this sweep raises its bound per domain tile of 32 blocks, not per block -- and the probes are exact quantised affine images of a d2 read
through an isometry (d2 + b, c - d2, d2 / 2 + b), so their winner is (g2, k) with E = 0 right behind a candidate with E <= 10^4.
Test infrastructure only: numpy and lsqtight's helpers; nothing here touches a GPU.

ER_SHARE and ESHIFT_CAUGHT are derived in tests/test_lsq_q_bound.py from the model (tests/lsqqmodel.py), never from a kernel,
and asserted there; tests/test_gpu_lsq_q.py applies them to the kernel."""
import functools

import numpy as np

import lsqtight as lt

I64 = np.int64
LO_LEVELS = np.arange(0, 16, 2)
HI_LEVELS = np.arange(240, 256, 2)

# The median share of Er that |acc - q| reaches on the winners of the probes, at least (per B; the two-level blocks of lsqtight
# give exactly 0).  It follows DRAW_SHARE below: a probe is an affine image of a block drawn with that share.
ER_SHARE = {4: 0.15, 8: 0.15, 16: 0.08}
# The smallest "lsq_q_eshift" k > 0 at which the model sweep loses the winner of a quarter of the probes or more, per (B, n_iso):
# 2^-k has to fall below the share of Er the winners are short by (minus the 2^-18 the safety factor and the probe's gap leave).
ESHIFT_CAUGHT = {(4, 1): 3, (4, 8): 2, (8, 1): 3, (8, 8): 3, (16, 1): 4, (16, 8): 3}


# A design block is drawn again until the f16 rounding of its normalised row SHORTENS the dot product with its own centred
# pixels by this share of Er or more (signed_share): the winner of its probes then sits below its exact q by that much, which
# is what a narrowed allowance ("lsq_q_eshift" > 0) turns into a pruned winner.  Rounding errors of a block with a handful of
# levels are strongly correlated, so such blocks are common (one draw in four to ten); the worst case of the derivation,
# every element half an ulp short, is 0.2 .. 0.36 of Er.
DRAW_SHARE = {4: 0.16, 8: 0.16, 16: 0.09}


def signed_share(d2, B):
    """(|acc| - |q|) / Er of the pair (range block = d2 itself, pool block = d2) on the model: negative when the rounded
    operand row gives less than the exact value."""
    import lsqqmodel as qm
    import qmodel
    d = np.asarray(d2, I64)[None]
    A, Bc = qm.a_rows(d, B), qm.b_columns(d, B, 1)
    return float((abs(qmodel.acc_exact(A, Bc)[0, 0]) - abs(qm.q_exact(d, Bc, B)[0, 0])) / qm.range_stats(d, B)["Er"][0])


def _build(B, n_iso, seed, attempt):
    rng = np.random.RandomState(200000 * attempt + 1000 * seed + 10 * B + n_iso)
    W = lt.SIDE[B]
    S, a, n = W // 2, B // 4, B * B
    Dw = (S - B) // a + 1
    iso = lt._iso_table(B)[:n_iso]
    sc = np.full((S, S // 2), 128, I64)
    tprows, tcols = S // B // 2, (S // 2) // B          # pairs one above the other: d1 is 4 Dw pool blocks, several domain tiles, before d2
    tiles = []
    for tr in range(tprows):
        for tp in range(tcols):
            while True:
                levels = np.concatenate([rng.choice(LO_LEVELS, 1 + rng.randint(3), replace=False),
                                         rng.choice(HI_LEVELS, 1 + rng.randint(3), replace=False)])
                d2 = levels[rng.randint(0, levels.size, size=n)].astype(I64)
                lo, hi = int(d2.min()), int(d2.max())
                if lo <= 14 and hi >= 240 and np.unique(d2).size >= 3 and signed_share(d2, B) <= -DRAW_SHARE[B]:
                    break
            d1 = d2.copy()
            p = rng.randint(n)
            d1[p] += 1 if (d1[p] == 0 or (d1[p] < 255 and rng.randint(2))) else -1
            x1, y = tp * B, 2 * tr * B
            sc[y:y + B, x1:x1 + B] = d1.reshape(B, B)
            sc[y + B:y + 2 * B, x1:x1 + B] = d2.reshape(B, B)
            tiles.append((((y + B) // a) * Dw + x1 // a, d2, lo, hi))
    img = np.zeros((W, W), I64)
    img[:, :W // 2] = np.repeat(np.repeat(sc, 2, axis=0), 2, axis=1)       # 2 x 2-constant cells: any averaging gives sc back
    Rw = W // B
    plan, used, t = [], set(), 0
    for ry in range(Rw):
        for rx in range(Rw // 2, Rw):
            g2, d2, lo, hi = tiles[t % len(tiles)]
            t += 1
            while True:
                k = rng.randint(n_iso)
                kind = rng.randint(3)
                if kind == 0:
                    b = rng.randint(-lo, 256 - hi)
                    qa, r = 100, d2 + b
                elif kind == 1:
                    b = rng.randint(hi, 256 + lo)
                    qa, r = -100, b - d2
                else:
                    b = rng.randint(-(lo // 2), 256 - hi // 2)
                    qa, r = 50, d2 // 2 + b
                key = (g2, k, kind, int(b))
                if key not in used:
                    used.add(key)
                    break
            assert r.min() >= 0 and r.max() <= 255
            img[ry * B:(ry + 1) * B, rx * B:(rx + 1) * B] = r[iso[k]].reshape(B, B)
            plan.append({"j": ry * Rw + rx, "g2": int(g2), "k": int(k), "qa": qa, "b": int(b), "copy": False})
    return img.astype(np.uint8), plan, tiles


@functools.lru_cache(maxsize=None)
def tight_multilevel(B, n_iso, seed=1):
    """(uint8 [W, W], probe table), W = lsqtight.SIDE[B].  Per probe: j, g2, k, qa, b, copy (always False: no same-block pairs
    here), E of (g2, k) and the number of candidates with E = 0 (a draw is thrown away unless every probe has exactly one)."""
    for attempt in range(50):
        img, plan, tiles = _build(B, n_iso, seed, attempt)
        pool = lt._pool(img, B, False)
        assert all((pool[g2][:, 0] == d2).all() for g2, d2, _, _ in tiles), "the scaled left half is not the design"
        s = lt.pair_sums(img, B, n_iso, False, rows=[p["j"] for p in plan])
        for i, p in enumerate(plan):
            p.update(E=int(s["E"][i, p["g2"], p["k"]]), zeros=int((s["E"][i] == 0).sum()), C=int(s["C"][i, p["g2"], p["k"]]),
                     V=int(s["V"][p["g2"]]), R=int(s["R"][i]))
        if all(p["E"] == 0 and p["zeros"] == 1 for p in plan):
            img.setflags(write=False)
            return img, tuple(plan)
    raise AssertionError("no draw with unique winners")
