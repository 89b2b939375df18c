"""Inputs that sit on the prune bound of the two fast least-squares sweeps (k_sweep_lsq_fast, DESIGN.md section 4.19, and
k_sweep_lsq_rgb_fast, section 4.20), a numpy float32 model of the bound's float chain, and inputs that reach the largest
integers of the search.  Test infrastructure only: numpy, Python ints and the oracle's pool; nothing here touches a GPU.

The sweeps skip a candidate when |C'| <= li, li = (int) fl(tau * s32'), tau from T = (S R - n E_best) / S (S = 10^4 grey,
10^6 RGB).  A skip is right while C'^2 <= T V'.  tight_gray / tight_rgb build images whose probe ranges have a winner with
C'^2 above T V' by a relative 2^-18 .. 2^-23 only -- E = 0 right behind a candidate that is one grey level off in one pixel --
so a bound that is wider than derived by a few 2^-18 skips the winner and the codebook changes.  li_model restates the chain;
WIDEN_CAUGHT is the widening it says the probes catch (derived in tests/test_lsq_bound.py, never from a kernel)."""
import functools
from fractions import Fraction

import numpy as np

I64 = np.int64
F32 = np.float32

SIDE = {4: 64, 8: 128, 16: 160}               # the smallest squares with a few hundred pool blocks: 841, 841, 289
# (NR, NC) of the fast instantiations: fic_fast_variant (grey), fic_lsq_rgb_variant (RGB: one range block per lane)
FAST = {False: {(4, 1): (4, 1), (4, 8): (1, 8), (8, 1): (2, 1), (8, 8): (1, 8), (16, 1): (2, 1), (16, 8): (1, 2)},
        True: {(4, 1): (1, 1), (4, 8): (1, 8), (8, 1): (1, 1), (8, 8): (1, 2)}}
SCALE = {False: 10 ** 4, True: 10 ** 6}       # E is this many times the squared error
QA_ONE = {False: 100, True: 1000}             # qa of a = 1

# The largest relative gap (C'^2 - T V') / (2 C'^2) of a probe.  With E_best = S (1 - 1/n) at most -- one pixel one level off --
# gap = n E_best / (2 S R) <= n / (2 R), R = channels * n^2 (hi - lo)^2 / 4, hi - lo >= 226: grey 2^-18.6 / 2^-20.6 / 2^-22.6,
# RGB a third of that.  A same-block probe (below) has an isometry copy of its own pool block as the near fit; a permutation
# that changes a block changes two pixels or more, so E_best = 2 S there and the gap is n / R: one bit more.  The RGB copies
# stay inside the table (2^-19.2, 2^-21.2), the grey ones do not (2^-17.6 .. 2^-21.6) and get twice the bound.
GAP_BOUND = {(False, 4): Fraction(1, 2 ** 18), (False, 8): Fraction(1, 2 ** 20), (False, 16): Fraction(1, 2 ** 22),
             (True, 4): Fraction(1, 2 ** 19), (True, 8): Fraction(1, 2 ** 21)}


def gap_bound(rgb, B, copy):
    return GAP_BOUND[(rgb, B)] * (2 if copy and not rgb else 1)


# The largest k at which li_model(widen=k) -- tau times 1 + 2^-k -- skips the winner of a quarter of the probes or more, per
# (RGB?, B, n_iso); tests/test_lsq_bound.py derives it from li_model and the probe tables and asserts this table.  The safety
# factor leaves 2^-18 and the probes' gap is far below that, so the first power of two above 2^-18 is caught.
WIDEN_CAUGHT = {(False, 4, 1): 17, (False, 4, 8): 17, (False, 8, 1): 17, (False, 8, 8): 17, (False, 16, 1): 17, (False, 16, 8): 17,
                (True, 4, 1): 17, (True, 4, 8): 17, (True, 8, 1): 17, (True, 8, 8): 17}


def li_model(Ti, V, widen=0, rgb=False):
    """li of the kernels for Ti = S T (an exact integer >= 0) and the candidate's V, elementwise: int64 -> f32, sqrt, times 0.01f
    (0.001f RGB), times the safety factor, times 1 + 2^-widen if widen, times fl32(sqrt((double) V)), truncated.  Every step is
    one IEEE operation rounded to nearest even, as __fmul_rn and a correctly rounded sqrtf are."""
    Ti, V = np.asarray(Ti, I64), np.asarray(V, I64)
    assert (Ti >= 0).all() and (V >= 0).all()
    tau = np.sqrt(Ti.astype(F32)) * F32(0.001 if rgb else 0.01)
    tau = tau * F32(0.99999618530273437500)
    if widen:
        tau = tau * F32(1.0 + 2.0 ** -widen)
    assert tau.dtype == F32
    s32 = np.sqrt(V.astype(np.float64)).astype(F32)
    return (tau * s32).astype(I64)


# ------------------------------------------------------------------------------------------------------------------------
# tight images
# ------------------------------------------------------------------------------------------------------------------------
def _iso_table(B):
    import qtmodel
    return qtmodel.iso_table(B)


def _two_level(rng, n, lo, hi):
    m = np.zeros(n, bool)
    m[rng.permutation(n)[:n // 2]] = True
    return np.where(m, hi, lo).astype(I64)


def _symmetric_two_level(rng, perm, lo, hi):
    """A block with n/2 pixels at lo and n/2 at hi that `perm` maps to itself (d[perm] == d), and a pixel of an orbit of two or
    more lo pixels: raising it by one level makes d[perm] differ from d in exactly two places."""
    n = perm.size
    seen, orbits = np.zeros(n, bool), []
    for p in rng.permutation(n):
        if not seen[p]:
            o, q = [], p
            while not seen[q]:
                seen[q] = True
                o.append(q)
                q = perm[q]
            orbits.append(o)
    orbits.sort(key=len, reverse=True)                 # stable: the draw's order within a size; the large orbits fill first
    bump = next(o for o in orbits if len(o) >= 2)      # stays at lo
    d, left = np.full(n, lo, I64), n // 2
    for o in orbits:
        if o is not bump and len(o) <= left:
            d[o] = hi
            left -= len(o)
    assert left == 0
    bump = bump[0]
    assert (d[perm] == d).all()
    return d, bump


def _build(B, n_iso, rgb, seed, attempt):
    nch = 3 if rgb else 1
    NC = FAST[rgb][(B, n_iso)][1]
    rng = np.random.RandomState(100000 * attempt + 1000 * seed + 10 * B + n_iso + (5 if rgb else 0))
    W = SIDE[B]
    S, a, n = W // 2, B // 4, B * B
    Dw = (S - B) // a + 1
    iso = _iso_table(B)[:n_iso]
    sc = np.full((S, S // 2, nch), 128, I64)           # the scaled left half; what no tile covers stays flat
    trows, tpairs = S // B, (S // 2) // B // 2
    tiles = []                                         # (pool index of d2, d2 [n, nch], lo, hi, same-block pair (k', k) or None)
    for tr in range(trows):
        for tp in range(tpairs):
            idx = tr * tpairs + tp
            lo = 2 * rng.randint(0, 8, size=nch)       # even levels: d2 / 2 is exact
            hi = 240 + 2 * rng.randint(0, 8, size=nch)
            copy = None
            if n_iso == 8 and idx % 3 == 2:
                # symmetric under the permutation that takes copy k' to copy k of the same NC group, but for one pixel pair: the
                # near fit of a probe read through k is the earlier copy k' of its own pool block
                kk = rng.randint(1, NC)
                k = NC * rng.randint(0, n_iso // NC) + kk
                k1 = k - 1 - rng.randint(0, kk)
                inv = np.argsort(iso[k])
                perm = iso[k1][inv]                     # d[iso[k1]] == d[iso[k]] iff d[perm] == d
                d2 = np.zeros((n, nch), I64)
                for ch in range(nch):
                    d2[:, ch], bump = _symmetric_two_level(rng, perm, lo[ch], hi[ch])
                    if ch == 0:
                        d2[bump, 0] += 1
                assert (d2[iso[k1]] != d2[iso[k]]).sum() == 2
                d1 = np.stack([_two_level(rng, n, lo[ch] + 1, hi[ch] - 1) for ch in range(nch)], axis=1)    # no fit at all
                copy = (k1, k)
            else:
                while True:                             # no isometry copy is another one or its negative: one exact fit only
                    d2 = np.stack([_two_level(rng, n, lo[ch], hi[ch]) for ch in range(nch)], axis=1)
                    m = [(d2[iso[k]] == hi).tobytes() for k in range(n_iso)] + [(d2[iso[k]] != hi).tobytes() for k in range(n_iso)]
                    if len(set(m)) == 2 * n_iso:
                        break
                d1 = d2.copy()
                p, ch = rng.randint(n), rng.randint(nch)
                up = d1[p, ch] == lo[ch]
                if rng.randint(2) and (d1[p, ch] > 0 if up else d1[p, ch] < 255):
                    up = not up                         # away from the other level where the byte has room
                d1[p, ch] += 1 if up else -1
            x1, y = 2 * tp * B, tr * B
            sc[y:y + B, x1:x1 + B] = d1.reshape(B, B, nch)
            sc[y:y + B, x1 + B:x1 + 2 * B] = d2.reshape(B, B, nch)
            tiles.append(((y // a) * Dw + (x1 + B) // a, d2, lo, hi, copy))
    img = np.zeros((W, W, nch), I64)
    img[:, :W // 2] = np.repeat(np.repeat(sc, 2, axis=0), 2, axis=1)       # 2 x 2-constant cells: any averaging gives sc back
    # probes: every range block of the right half, the tiles in turn, no (tile, k, map) twice
    Rw = W // B
    plan, used, t = [], set(), 0
    for ry in range(Rw):
        for rx in range(Rw // 2, Rw):
            g2, d2, lo, hi, copy = tiles[t % len(tiles)]
            t += 1
            while True:
                k = copy[1] if copy else rng.randint(n_iso)
                kind = rng.randint(2 if copy else 3)
                if kind == 0:                           # r = d2 + b
                    b = np.array([rng.randint(-lo[ch], 256 - hi[ch]) for ch in range(nch)])
                    qa, r = QA_ONE[rgb], d2 + b
                elif kind == 1:                         # r = c - d2
                    b = np.array([rng.randint(hi[ch], 256 + lo[ch]) for ch in range(nch)])
                    qa, r = -QA_ONE[rgb], b - d2
                else:                                   # r = d2 / 2 + b
                    b = np.array([rng.randint(-(lo[ch] // 2), 256 - hi[ch] // 2) for ch in range(nch)])
                    qa, r = QA_ONE[rgb] // 2, d2 // 2 + b
                key = (g2, k, kind, tuple(b))
                if key not in used:
                    used.add(key)
                    break
            assert r.min() >= 0 and r.max() <= 255
            img[ry * B:(ry + 1) * B, rx * B:(rx + 1) * B] = _read(r, iso[k], B, nch)
            plan.append({"j": ry * Rw + rx, "g2": int(g2), "k": int(k), "qa": qa, "b": [int(v) for v in b], "copy": copy is not None})
    return img.astype(np.uint8), plan, tiles


def _read(r_of_d2, perm, B, nch):
    """The range block that equals the map of d2 read through the isometry: position p holds the value made from d2[perm[p]]."""
    return r_of_d2[perm].reshape(B, B, nch)


def _pool(img, B, rgb):
    """int64 [N_d, n, channels] of the oracle's pool (createCodebuch / createCodebuchRGB)."""
    if rgb:
        import rgblsqmodel as lm
        from oracle import fic_oracle as fo
        h, w = img.shape[:2]
        return lm._pool(fo.rgb_to_argb(img), w, h, B)
    import lsqmodel as lm
    return lm._pool(img, B)[:, :, None]


def _blocks(img, B):
    h, w, nch = img.shape
    return img.astype(I64).reshape(h // B, B, w // B, B, nch).transpose(0, 2, 1, 3, 4).reshape(-1, B * B, nch)


def pair_sums(img, B, n_iso, rgb, rows=None):
    """The exact sums of every (range block, pool block, isometry) of a full search, int64: dict with C, V, R [rows, N_d, n_iso]
    (V [N_d], R [rows]) and E [rows, N_d, n_iso] of the quantised fit.  img uint8 [H, W] or [H, W, 3]."""
    img3 = img if img.ndim == 3 else img[:, :, None]
    n = B * B
    pool = _pool(img if rgb else img3[:, :, 0], B, rgb)
    r = _blocks(img3, B)
    if rows is not None:
        r = r[rows]
    iso = _iso_table(B)[:n_iso]
    dk = np.stack([pool[:, iso[k], :] for k in range(n_iso)], axis=1)                      # [N_d, n_iso, n, nch]
    S_rd = (r.reshape(r.shape[0], -1).astype(np.float64) @ dk.reshape(-1, dk.shape[2] * dk.shape[3]).astype(np.float64).T)
    S_rd = np.rint(S_rd).astype(I64).reshape(r.shape[0], pool.shape[0], n_iso)            # exact: below 2^53
    S_r, S_d = r.sum(axis=1), pool.sum(axis=1)                                             # [rows, nch], [N_d, nch]
    S_rr, S_dd = (r * r).sum(axis=(1, 2)), (pool * pool).sum(axis=(1, 2))
    C = n * S_rd - (S_r[:, None, :] * S_d[None, :, :]).sum(axis=-1)[:, :, None]
    V = n * S_dd - (S_d * S_d).sum(axis=1)
    R = n * S_rr - (S_r * S_r).sum(axis=1)
    if rgb:
        import rgblsqmodel as lm
        qa, t = lm.fit(n, S_r[:, None, None, :], S_d[None, :, None, :], S_dd[None, :, None], S_rd)
        E = lm.closed_form(n, S_r[:, None, None, :], S_rr[:, None, None], S_d[None, :, None, :], S_dd[None, :, None], S_rd, qa, t)
    else:
        import lsqmodel as lm
        qa, qb = lm.fit(n, S_r[:, 0, None, None], S_d[None, :, 0, None], S_dd[None, :, None], S_rd)
        E = lm.closed_form(n, S_r[:, 0, None, None], S_rr[:, None, None], S_d[None, :, 0, None], S_dd[None, :, None], S_rd, qa, qb)
    return {"C": C, "V": V, "R": R, "E": E, "n_dd": n * S_dd}


@functools.lru_cache(maxsize=None)
def _tight(B, n_iso, rgb, seed):
    # At B = 4 a pool block that straddles two tiles now and then fits a probe exactly as well; such a draw is thrown away, so
    # that every probe has one candidate with E = 0 (tests/test_lsq_bound.py asserts it).  Decided on the model's sums alone.
    for attempt in range(50):
        img, table = _tight_draw(B, n_iso, rgb, seed, attempt)
        if all(p["E"] == 0 and p["zeros"] == 1 for p in table):
            return img, table
    raise AssertionError("no draw with unique winners")


def _tight_draw(B, n_iso, rgb, seed, attempt):
    img, plan, tiles = _build(B, n_iso, rgb, seed, attempt)
    if not rgb:
        img = img[:, :, 0]
    NR, NC = FAST[rgb][(B, n_iso)]
    n, S = B * B, SCALE[rgb]
    pool = _pool(img, B, rgb)
    for g2, d2, lo, hi, copy in tiles:
        assert (pool[g2] == d2).all(), "the scaled left half is not the design"
    s = pair_sums(img, B, n_iso, rgb, rows=[p["j"] for p in plan])
    kk = np.arange(n_iso)
    for i, p in enumerate(plan):
        g2, k = p["g2"], p["k"]
        E = s["E"][i]
        # what the wave that holds copy k has seen before (g2, k) in a one-chunk ascending scan: the isometries of its group
        mine = (kk // NC) == (k // NC)
        before = E[:g2][:, mine].min() if g2 else None
        same = E[g2][mine & (kk < k)]
        if same.size:
            before = same.min() if before is None else min(before, same.min())
        E_best = int(before)
        C, V, R = int(s["C"][i, g2, k]), int(s["V"][g2]), int(s["R"][i])
        Ti = S * R - n * E_best
        p.update(E=int(E[g2, k]), zeros=int((E == 0).sum()), E_best=E_best, C=C, V=V, R=R, Ti=Ti,
                 gap=Fraction(S * C * C - Ti * V, 2 * S * C * C), slot=(p["j"] // 64) % NR)
    img.setflags(write=False)
    return img, tuple(plan)


def tight_gray(B, n_iso, seed=1):
    """(uint8 [W, W], probe table) for the grey fast sweep at block size B, W = SIDE[B].  The left half of the image is domain
    material in 2 x 2-constant cells: the scaled image there is a design of B x B tiles in pairs d1, d2 (d1 earlier in pool
    order); d2 has n/2 pixels at an even level lo <= 14 and n/2 at an even level hi >= 240, d1 is d2 with one pixel moved by one
    level.  With n_iso = 8 every third pair is a same-block pair instead: d2 is symmetric under the permutation between two
    isometries k' < k of one register-resident group but for one pixel raised by one level, and d1 is unrelated.  The right half
    holds the probes: each an exact quantised affine image of a d2 read through an isometry k -- d2 + b (qa 100), c - d2 (-100),
    d2 / 2 + b (50) -- so its winner is (g2, k) with E = 0.  Per probe the table has j, g2, k, copy (same-block?), slot
    ((j // 64) % NR), E and the number of candidates with E = 0, E_best just before (g2, k) in a one-chunk ascending scan over
    the isometries that share k's group, C, V, R, Ti = S T of that moment and the exact gap (C^2 - T V) / (2 C^2)."""
    return _tight(B, n_iso, False, seed)


def tight_rgb(B, n_iso, seed=1):
    """tight_gray for the joint-RGB fast sweep (B = 4, 8): uint8 [W, W, 3], levels and positions of their own per channel, one
    qa (1000, -1000, 500) and an integer b per channel, d1 one level off in one pixel of one channel."""
    return _tight(B, n_iso, True, seed)


def chunk_starts(Nd, chunks, rgb):
    """First pool block of every chunk under the option "chunks" = chunks (the grey sweep takes its blocks in pairs)."""
    L = (Nd + chunks - 1) // chunks
    if not rgb:
        L = (L + 1) & ~1
    return list(range(0, Nd, L))


def cutting_chunks(B, table, rgb):
    """The smallest "chunks" > 1 that cuts the pool between the d1 tile (B / (B / 4) = 4 pool blocks before d2) and the d2 tile
    of a pair probe: the bound starts afresh right before the winner."""
    W = SIDE[B]
    Dw = (W // 2 - B) // (B // 4) + 1
    for chunks in range(2, 65):
        starts = chunk_starts(Dw * Dw, chunks, rgb)
        if any(not p["copy"] and any(p["g2"] - 4 < s <= p["g2"] for s in starts) for p in table):
            return chunks
    raise AssertionError("no chunk count cuts a pair")


# ------------------------------------------------------------------------------------------------------------------------
# full-range images
# ------------------------------------------------------------------------------------------------------------------------
HALVES_SEED = 7
# the full-range cases of the GPU tests, square images: (side, B, perturbed share) and (side, B, equal channels, perturbed share);
# 48 x 48 at B = 16 has a 3 x 3 pool: the full search through the windowed entry at wK = 3
GRAY_FULL = [(160, 16, 0.0), (128, 8, 0.0), (64, 4, 0.1)]
RGB_FULL = [(160, 16, False, 0.0), (160, 16, True, 0.0), (128, 8, False, 0.0), (64, 4, False, 0.1), (48, 16, True, 0.0)]


def halves_image(w, h, B, channels, seed, equal=False, perturb=0.0):
    """uint8 [h, w] (channels = 1) or [h, w, 3]: pixels 0 or 255 in 4 x 4 pixel cells, about half of each, independently per
    channel or (equal) the same in the three channels, so that the scaled image and every pool block are binary and V, R and C
    come close to their largest values, channels * n^2 255^2 / 4.  The cells start at pixel 2, not 0, so that range blocks of
    every size mix cells.  Two range blocks are planted: the last one is pool block 0 (the image's top left corner at half
    size) and the one before it is 255 minus that, so some pair has C = V and some C = -V whatever the seed draws.
    perturb: that share of the 2 x 2 pixel cells (the pixels of the scaled image) moves by 1 .. 40 levels towards the middle.
    At B = 4 a range block is four such cells, the half-size picture of the four 4 x 4 cells it touches: without the
    perturbation every block there has an exact fit (E = 0) and the comparison of qa, qb and E would say little."""
    rng = np.random.RandomState(seed)
    nch = 1 if channels == 1 else 3
    cells = rng.randint(0, 2, size=(h // 4 + 1, w // 4 + 1, 1 if equal else nch)) * 255
    cells = np.broadcast_to(cells, cells.shape[:2] + (nch,))
    half = np.repeat(np.repeat(cells, 2, axis=0), 2, axis=1)[1:1 + h // 2, 1:1 + w // 2].copy()      # the scaled image
    if perturb:
        hit = rng.random_sample(half.shape[:2] + (1 if equal else nch,)) < perturb
        step = rng.randint(1, 41, size=hit.shape)
        half = np.where(hit, np.abs(half - step), half)
    img = np.repeat(np.repeat(half, 2, axis=0), 2, axis=1)
    d0 = half[:B, :B].copy()                                                              # pool block 0
    img[h - B:, w - B:] = d0
    img[h - B:, w - 2 * B:w - B] = 255 - d0
    img = img.astype(np.uint8)
    return img[:, :, 0] if channels == 1 else img
