"""Tight inputs for the matrix-core joint-RGB least-squares sweep (k_sweep_lsq_rgb_q), B = 4 / 8 / 16.

Two families, both with probes whose winner has E = 0 right behind a near fit (lsqtight's construction):
  * two-level: lsqtight.tight_rgb at B = 4 / 8 (d1 four pool blocks before d2, mostly the SAME domain tile of 32 blocks: the
    second stage's round-by-round tau is what they sit on), and at B = 16, where lsqtight has no colour table, two_level16 built
    here on 160 x 160 with the layout below.  With levels of their own per channel the normalised rows are not exact in f16, so
    they use some of Er on either side (up to 0.3 of it at B = 4; tests/test_rgb_lsq_q_bound.py measures it on the model).
  * multi-level: the design of tests/lsqqtight.py for three channels.  Every pixel of a design block d2 is drawn per channel from
    a few even levels <= 14 or >= 240; d1 is d2 with one pixel of one channel one level off and lies one block ROW higher, 4 Dw
    pool blocks and so several domain tiles earlier, because this sweep raises theta per domain tile.  A block is drawn again
    until the f16 rounding of its normalised row SHORTENS the dot product with its own centred pixels by DRAW_SHARE of Er or
    more: the winner of its probes then sits below its exact q by that much, which a narrowed allowance ("lsq_q_eshift" > 0)
    turns into a pruned winner.
The probes are exact quantised affine images of a d2 read through an isometry k with ONE a for the three channels and an integer
b per channel (d2 + b: qa 1000, c - d2: -1000, d2 / 2 + b: 500).
Test infrastructure only: numpy and lsqtight's helpers; nothing here touches a GPU.

ESHIFT_CAUGHT and WIDEN_CAUGHT are derived in tests/test_rgb_lsq_q_bound.py from the model (tests/rgblsqqmodel.py), never from
a kernel, and asserted there; tests/test_gpu_rgb_lsq_q.py applies them to the kernel."""
import functools

import numpy as np

import lsqtight as lt

I64 = np.int64
LO_LEVELS = np.arange(0, 16, 2)
HI_LEVELS = np.arange(240, 256, 2)
SIDE = lt.SIDE                                  # 64, 128, 160: 841, 841, 289 pool blocks

# A multi-level design block is accepted when (|acc| - |q|) / Er of the pair (the block, itself) is at most minus this.  Er's
# coefficient is 1.13e-3 / 1.56e-3 / 2.45e-3 ||b|| at B = 4 / 8 / 16 (most of it the subnormal term), the f16 rounding of a row can
# reach 2^-12 .. 2^-11 ||b|| = 0.1 .. 0.4 of that when every element errs the same way; blocks of a handful of levels do so often.
DRAW_SHARE = {4: 0.13, 8: 0.10, 16: 0.075}
# The smallest "lsq_q_eshift" k > 0 at which the model sweep loses the winner of a quarter of the multi-level probes or more, per
# (B, n_iso): 2^-k has to fall below the share of Er the winners are short by.
ESHIFT_CAUGHT = {(4, 1): 3, (4, 8): 3, (8, 1): 4, (8, 8): 4, (16, 1): 4, (16, 8): 4}
# A k at which the model sweep under tau times 1 + 2^-k loses the winner of two-level probes (at least one; at B = 4 / 8, where
# near fit and winner mostly share a domain tile, only those whose near fit is evaluated in an earlier round or tile feel it): the
# safety factor leaves 2^-18 and the probes' gap is far below it, so the first power of two above 2^-18.
WIDEN_CAUGHT = {(4, 1): 17, (4, 8): 17, (8, 1): 17, (8, 8): 17, (16, 1): 17, (16, 8): 17}


def signed_share(d2, B):
    """(|acc| - |q|) / Er of the pair (range block = d2 itself, pool block = d2), d2 int [n, 3], on the model: negative when the
    rounded operand row gives less than the exact value."""
    import qmodel
    import rgblsqqmodel as qm
    d = np.asarray(d2, I64)[None]
    A, Bc = qm.a_rows(d, B), qm.b_columns(d, B, 1)
    return float((abs(qmodel.acc_exact(A, Bc)[0, 0]) - abs(qm.q_exact(d, Bc, B)[0, 0])) / qm.range_stats(d, B)["Er"][0])


def _draw_block(rng, n, multilevel):
    d2 = np.zeros((n, 3), I64)
    for ch in range(3):
        if multilevel:
            levels = np.concatenate([rng.choice(LO_LEVELS, 1 + rng.randint(3), replace=False),
                                     rng.choice(HI_LEVELS, 1 + rng.randint(3), replace=False)])
            d2[:, ch] = levels[rng.randint(0, levels.size, size=n)]
        else:
            d2[:, ch] = lt._two_level(rng, n, 2 * rng.randint(0, 8), 240 + 2 * rng.randint(0, 8))
    return d2


def _build(B, n_iso, seed, attempt, multilevel):
    rng = np.random.RandomState(300000 * attempt + 1000 * seed + 10 * B + n_iso + (3 if multilevel else 0))
    W = SIDE[B]
    S, a, n = W // 2, B // 4, B * B
    Dw = (S - B) // a + 1
    iso = lt._iso_table(B)[:n_iso]
    sc = np.full((S, S // 2, 3), 128, I64)
    tprows, tcols = S // B // 2, (S // 2) // B          # pairs one above the other: d1 is 4 Dw pool blocks, several domain tiles, before d2
    tiles = []
    for tr in range(tprows):
        for tp in range(tcols):
            while True:
                d2 = _draw_block(rng, n, multilevel)
                lo, hi = d2.min(0), d2.max(0)
                if (lo > 14).any() or (hi < 240).any():
                    continue
                if not multilevel or (min(np.unique(d2[:, ch]).size for ch in range(3)) >= 2 and np.unique(d2).size >= 5
                                      and signed_share(d2, B) <= -DRAW_SHARE[B]):
                    break
            d1 = d2.copy()
            p, ch = rng.randint(n), rng.randint(3)
            d1[p, ch] += 1 if (d1[p, ch] == 0 or (d1[p, ch] < 255 and rng.randint(2))) else -1
            x1, y = tp * B, 2 * tr * B
            sc[y:y + B, x1:x1 + B] = d1.reshape(B, B, 3)
            sc[y + B:y + 2 * B, x1:x1 + B] = d2.reshape(B, B, 3)
            tiles.append((((y + B) // a) * Dw + x1 // a, d2, lo, hi))
    img = np.zeros((W, W, 3), I64)
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
                    b = np.array([rng.randint(-lo[ch], 256 - hi[ch]) for ch in range(3)])
                    qa, r = 1000, d2 + b
                elif kind == 1:
                    b = np.array([rng.randint(hi[ch], 256 + lo[ch]) for ch in range(3)])
                    qa, r = -1000, b - d2
                else:
                    b = np.array([rng.randint(-(lo[ch] // 2), 256 - hi[ch] // 2) for ch in range(3)])
                    qa, r = 500, d2 // 2 + b
                key = (g2, k, kind, tuple(int(v) for v in b))
                if key not in used:
                    used.add(key)
                    break
            assert r.min() >= 0 and r.max() <= 255
            img[ry * B:(ry + 1) * B, rx * B:(rx + 1) * B] = lt._read(r, iso[k], B, 3)
            plan.append({"j": ry * Rw + rx, "g2": int(g2), "k": int(k), "qa": qa, "b": [int(v) for v in b], "copy": False,
                         "g1": int(g2) - 4 * Dw})
    return img.astype(np.uint8), plan, tiles


@functools.lru_cache(maxsize=None)
def _tight(B, n_iso, seed, multilevel):
    for attempt in range(50):
        img, plan, tiles = _build(B, n_iso, seed, attempt, multilevel)
        pool = lt._pool(img, B, True)
        assert all((pool[g2] == d2).all() for g2, d2, _, _ in tiles), "the scaled left half is not the design"
        s = lt.pair_sums(img, B, n_iso, True, rows=[p["j"] for p in plan])
        for i, p in enumerate(plan):
            p.update(E=int(s["E"][i, p["g2"], p["k"]]), zeros=int((s["E"][i] == 0).sum()), C=int(s["C"][i, p["g2"], p["k"]]),
                     V=int(s["V"][p["g2"]]), R=int(s["R"][i]), E_near=int(s["E"][i, p["g1"]].min()))
        if all(p["E"] == 0 and p["zeros"] == 1 for p in plan):
            img.setflags(write=False)
            return img, tuple(plan)
    raise AssertionError("no draw with unique winners")


def tight_multilevel(B, n_iso, seed=1):
    """(uint8 [W, W, 3], probe table), W = SIDE[B].  Per probe: j, g2, k, qa, b [3], g1 (the near fit's pool block, 4 Dw before
    g2), E of (g2, k) and the number of candidates with E = 0 (a draw is thrown away unless every probe has exactly one), C, V, R
    of the winning pair and E_near, the smallest E over the isometries of g1."""
    return _tight(B, n_iso, seed, True)


def two_level16(n_iso, seed=1):
    """The two-level family at B = 16 (160 x 160), which lsqtight does not have for colour: the layout above, every channel of a
    design block n / 2 pixels at an even level <= 14 and n / 2 at an even level >= 240."""
    return _tight(16, n_iso, seed, False)


def two_level(B, n_iso, seed=1):
    return two_level16(n_iso, seed) if B == 16 else lt.tight_rgb(B, n_iso, seed)


def tie_image():
    """(uint8 [32, 32, 3], probe range block j): B = 4.  The scaled image has period 3 along x (2 x 2-constant cells), so pool
    blocks d and d + 3 of a pool row are the same block; the last range block is pool block 1 itself.  Its exact hits (E = 0) in
    the first domain tile are the pool blocks 1, 4, 7, 10 and not block 0: the winner is candidate 1 * n_iso, which a sweep finds
    only if an exact hit in a LATER pool block of the tile under test does not end the search (in the kernel's order of
    evaluation pool block 4 comes before pool block 1)."""
    W, S = 32, 16
    cols = np.array([[10, 200, 90], [250, 30, 140], [60, 120, 220]], I64)          # [x % 3, channel]
    rows = np.array([0, 3, 1, 5, 2, 0, 4, 1, 3, 2, 5, 0, 1, 4, 2, 3], I64)          # no symmetry along y either
    sc = cols[np.arange(S) % 3][None, :, :] + rows[:, None, None]
    img = np.repeat(np.repeat(sc, 2, axis=0), 2, axis=1)
    img[W - 4:, W - 4:] = sc[0:4, 1:5]
    img = img.astype(np.uint8)
    img.setflags(write=False)
    return img, (W // 4) ** 2 - 1
