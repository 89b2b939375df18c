"""Quadtree encode by rate-distortion pruning on the GPU against the numpy model (tests/qtrdmodel.py):
the key kernel and the weighted select alone through their hooks, and the RD entries of every quadtree format under both
search criteria: the tree against the model's on the library's own per-level SSE, the rows against the fixed-B encode of each
level, lambda and the statistics against the model, the three goals by their defining properties, the threshold budget at the
same size (which can never be better), and the leaf tables through the stream writers and decoders."""
import bisect
import os

import numpy as np
import pytest

import geomcases as gc
import isostreammodel as im
import qtbudgetmodel as qb
import qtmodel as qm
import qtrdmodel as rd
import qtrgbmodel as qr

import fic_amd
from fic_amd import capi, synth

pytestmark = pytest.mark.gpu

INF = float("inf")
LEVELS = [(16, 4), (8, 4), (16, 8)]


# ---- the key kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B_max,B_min", LEVELS)
@pytest.mark.parametrize("w,h", [(32, 32), (64, 48), (256, 256)])
def test_keys_hook_matches_the_model(w, h, B_max, B_min):
    """4 to 256 top-level blocks (a wave partly filled, one workgroup, several with the blocks of level 1), every ladder, SSE
    arrays at both ends of the 32-bit range and seeded random ones."""
    for name, sse in rd.adversarial(w, h, B_max, B_min, seed=w + h).items():
        e, G = rd.keys_gains(sse, B_max, B_min)
        keys, gains = capi.debug_qt_rd_keys(sse, w, h, B_max, B_min)
        assert keys.dtype == np.uint32 and gains.dtype == np.int64 and keys.shape == e.shape
        bad = np.nonzero((keys.astype(np.int64) != e) | (gains != G))[0]
        assert bad.size == 0, f"{name} {w}x{h} {B_max}->{B_min}: block {bad[:5]}: keys {keys[bad[:5]]} gains {gains[bad[:5]]}, model {e[bad[:5]]} {G[bad[:5]]}"


# ---- the weighted select ----------------------------------------------------------------------------------------------------------
def _boundaries(keys, gains):
    """[(boundary, #{key > boundary}, their gain)] over the distinct keys in descending order, then 0."""
    keys, gains = np.asarray(keys).astype(np.int64), np.asarray(gains).astype(np.int64)
    order = np.argsort(-keys, kind="stable")
    ks, cum = keys[order], np.concatenate([[0], np.cumsum(gains[order])])
    first = np.nonzero(np.r_[True, ks[1:] != ks[:-1]])[0]
    out = [(int(ks[i]), int(i), int(cum[i])) for i in first]
    if ks[-1] != 0:
        out.append((0, int(ks.size), int(cum[-1])))
    return out


def _pair_sets():
    rng = np.random.default_rng(20261020)
    sets = {}
    for n in (1, 255, 256, 257):
        sets[f"random-n{n}"] = (rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32), rng.integers(0, 1 << 33, n))
        sets[f"few-keys-n{n}"] = (rng.choice(np.array([0, 7, 0x01020304, 0xFFFFFFFF], np.uint32), n), rng.integers(0, 1000, n))
    sets["equal-n257"] = (np.full(257, 0x01020304, np.uint32), rng.integers(0, 1 << 20, 257))       # one bin in every pass
    sets["all-zero-n70"] = (np.zeros(70, np.uint32), rng.integers(1, 100, 70))
    sets["all-max-n65"] = (np.full(65, 0xFFFFFFFF, np.uint32), rng.integers(1, 100, 65))
    sets["zero-gains-n256"] = (rng.integers(0, 1 << 32, 256, dtype=np.uint64).astype(np.uint32), np.zeros(256, np.int64))
    sets["top-byte-n300"] = ((rng.integers(0, 256, 300, dtype=np.uint64) << 24).astype(np.uint32) | np.uint32(0x00ABCDEF), rng.integers(0, 1 << 40, 300))
    sets["bottom-byte-n300"] = (rng.integers(0, 256, 300, dtype=np.uint64).astype(np.uint32) | np.uint32(0x12345600), rng.integers(0, 1 << 40, 300))
    sets["full-bin-n1024"] = (np.repeat(rng.integers(0, 1 << 32, 4, dtype=np.uint64).astype(np.uint32), 256), rng.integers(0, 50, 1024))
    # many workgroups; 2000 distinct 32-bit keys, so that every cumulated value can be asked for
    sets["random-n20001"] = (rng.choice(rng.integers(0, 1 << 32, 2000, dtype=np.uint64).astype(np.uint32), 20001), rng.integers(0, 1 << 34, 20001))
    # real pairs: gains of either sign, the cumulated gain still never falls from one distinct key to the next
    for name, (w, B_max, B_min) in {"real-n1280": (256, 16, 4), "real-n256": (128, 8, 4), "real-n20480": (1024, 16, 4)}.items():
        sse = rd.adversarial(w, w, B_max, B_min, seed=5)["random-decaying"]
        if w == 1024:       # coarse SSE values: a few thousand distinct keys among the 20480, the rest ties
            sse = {B: ((v.astype(np.uint64) * 40 >> int(v.max()).bit_length()) << (int(v.max()).bit_length() - 5)).astype(np.uint32) for B, v in sse.items()}
        e, G = rd.keys_gains(sse, B_max, B_min)
        sets[name] = (e.astype(np.uint32), G)
        assert (G < 0).any() and e.size == int(name.split("n")[-1])
    return sets


PAIR_SETS = _pair_sets()


@pytest.mark.parametrize("name", list(PAIR_SETS))
def test_weighted_select_matches_the_model(name):
    keys, gains = PAIR_SETS[name]
    bounds = _boundaries(keys, gains)
    sums = [s for _, _, s in bounds]
    assert all(a <= b for a, b in zip(sums, sums[1:])), "the precondition of the select"
    total = sums[-1]
    needs = {-5, 0, 1, total - 1, total, total + 1, total + (1 << 40)}
    for s in sums:                                              # each cumulated value and the one after it
        needs |= {s, s + 1}
    for need in sorted(needs):
        want = bounds[min(bisect.bisect_left(sums, need), len(bounds) - 1)]      # the first boundary whose sum reaches need, else the last
        got = capi.debug_qt_select_weighted(keys, gains, need)
        assert got == want, f"{name}: need {need}: {got}, model {want}"
        if keys.size <= 300 and need in (0, 1, total, total + 1):
            assert want == rd.select_weighted(keys, gains, need)
    if keys.size > 1:
        assert capi.debug_qt_select_weighted(keys, gains, -(1 << 62))[0] == int(keys.max())


# ---- the entries ------------------------------------------------------------------------------------------------------------------
class _Codec:
    """One quadtree format on one image: the fixed-threshold, budget and RD entries, the SSE hook, the model's SSE of a level's
    rows, the stream writer, the decoder and the model's decoder."""

    def __init__(self, codec, argb, w, h, wK):
        self.codec, self.w, self.h, self.wK = codec, w, h, wK
        self.argb = np.ascontiguousarray(argb, np.int32).reshape(-1)
        self.orig = qr.channels(self.argb, w, h)
        self.n_iso = int(codec[-1]) if codec[-1] in "18" else 1
        self.grey = codec.startswith("grey")
        if self.grey:
            self.g = np.ascontiguousarray(self.orig[..., 0].astype(np.uint8))
        self.cols = 7 if self.grey else (8 if codec == "rgb" else 9)

    def _head(self, B_max, B_min):
        if self.grey:
            return (self.g, B_max, B_min, self.wK, self.n_iso)
        return (self.argb, self.w, self.h, B_max, B_min, self.wK) + (() if self.codec == "rgb" else (self.n_iso,))

    def _fn(self, suffix):
        return getattr(capi, {"g": "encode_gray_quadtree", "r": "encode_rgb_quadtree"}[self.codec[0]] + ("_iso" if self.codec.startswith("rgbiso") else "") + suffix)

    def fixed(self, B_max, B_min, t, search):
        return self._fn("")(*self._head(B_max, B_min), t, search=search)

    def budget(self, B_max, B_min, M):
        return self._fn("_budget")(*self._head(B_max, B_min), max_leaves=M)

    def rd(self, B_max, B_min, search, **goal):
        return self._fn("_rd")(*self._head(B_max, B_min), search=search, **goal)

    def sse_hook(self, B_max, B_min):
        if self.grey:
            return capi.debug_quadtree_sse(self.g, B_max, B_min, self.wK, self.n_iso)
        if self.codec == "rgb":
            return capi.debug_rgb_quadtree_sse(self.argb, self.w, self.h, B_max, B_min, self.wK)
        return capi.debug_rgb_quadtree_iso_sse(self.argb, self.w, self.h, B_max, B_min, self.wK, self.n_iso)

    def rows_sse(self, B, tab):
        wk = qm.level_wk(self.w, self.h, B, self.wK)
        if self.grey:
            return qm.collage_sse(self.g, B, wk, tab[:, 3:6], tab[:, 6])
        if self.codec == "rgb":
            return qr.collage_sse(self.orig, B, wk, tab[:, 3:8])
        return im.collage_sse(self.orig, B, wk, tab[:, 3:8], tab[:, 8])

    def level_tables(self, B_max, B_min, search):
        """{B: the rows of the fixed-B encode of level B as a leaf table in scanline order}, from the fixed-threshold entry: every
        block whole (+inf), every block split (-1), and the middle level as the top of the ladder below."""
        out = {}
        for B in qm.levels(B_max, B_min):
            t = self.fixed(B_max, B_min, INF, search) if B == B_max else (self.fixed(B_max, B_min, -1.0, search) if B == B_min else self.fixed(B, B_min, INF, search))
            assert (t[:, 2] == B).all() and len(t) == (self.w // B) * (self.h // B)
            tab = np.zeros_like(t)
            tab[(t[:, 1] // B) * (self.w // B) + t[:, 0] // B] = t
            out[B] = tab
        return out

    def sse(self, B_max, B_min, search, tables):
        """The per-level SSE the entry decides on: the library's own arrays (reference criterion: the SSE hook), or the model's
        collage SSE of the library's fixed-B rows (least squares, which the hooks do not take)."""
        if search == "reference":
            return {B: v.astype(np.int64) for B, v in self.sse_hook(B_max, B_min).items()}
        return {B: self.rows_sse(B, tables[B]).astype(np.int64) for B in tables}

    def stream(self, leaves, B_max, B_min):
        """(run, the library's decode at zoom 1 as (rgb or grey array, avgError, iterations), the model's decoder)."""
        if self.grey:
            run = fic_amd.write_run_quadtree(leaves, self.w, self.h, B_max, B_min, self.wK, self.n_iso)
            return run, fic_amd.decode_quadtree_run(run), qm.decode
        if self.codec == "rgb":
            run = fic_amd.write_run_rgb_quadtree(leaves, self.w, self.h, B_max, B_min, self.wK)
            img, avg, it = fic_amd.decode_rgb_quadtree_run(run)
            return run, (qr.channels(img, self.w, self.h), avg, it), qr.decode
        run = fic_amd.write_run_rgb_quadtree_iso(leaves, self.w, self.h, B_max, B_min, self.wK)
        img, avg, it = fic_amd.decode_rgb_quadtree_iso_run(run)
        return run, (qr.channels(img, self.w, self.h), avg, it), im.decode_qt


def _want_table(tree, tables, w):
    return np.array([tables[B][(y // B) * (w // B) + x // B] for x, y, B in tree], np.int32)


def _check_rd(E, sse, tables, B_max, B_min, search, what, **goal):
    """One RD call against the model on `sse`: lambda, the tree, the rows, the statistics.  Returns (leaves, lam, stats)."""
    kind, value = next(iter(goal.items()))
    lam_want = rd.choose(sse, E.w, E.h, B_max, B_min, {"lam": rd.GOAL_LAMBDA, "max_leaves": rd.GOAL_LEAVES, "max_sse": rd.GOAL_SSE}[kind], value)
    leaves, lam, stats = E.rd(B_max, B_min, search, **goal)
    print(f"{what}: {kind} = {value}: lambda {lam}, {len(leaves)} leaves, stats {stats.tolist()}")
    assert lam == lam_want, f"{what}: {kind} = {value}: lambda {lam}, model {lam_want}"
    want = _want_table(rd.tree(sse, E.w, E.h, B_max, B_min, lam_want), tables, E.w)
    assert leaves.shape == want.shape and leaves.shape[1] == E.cols, f"{what}: {kind} = {value}: {len(leaves)} leaves, model {len(want)}"
    assert (leaves[:, :3] == want[:, :3]).all(), f"{what}: {kind} = {value}: the tree"
    assert (leaves[:, 3:] == want[:, 3:]).all(), f"{what}: {kind} = {value}: the rows against the fixed-B encodes"
    n, d = rd.tree_nd(sse, B_max, B_min, lam_want)
    assert (stats == qb.tree_stats(sse, leaves, B_max)).all() and int(stats[0]) == d and int(stats[1:].sum()) == n == len(leaves)
    return leaves, lam, stats


def _check_all_goals(E, B_max, B_min, search, what, decode_model):
    w, h = E.w, E.h
    tables = E.level_tables(B_max, B_min, search)
    sse = E.sse(B_max, B_min, search, tables)
    n_top, n_max, s_top = (w // B_max) * (h // B_max), (w // B_min) * (h // B_min), int(sse[B_max].sum())
    e, G = rd.keys_gains(sse, B_max, B_min)
    bounds = sorted(set(e.tolist()) | {0})
    go = lambda **goal: _check_rd(E, sse, tables, B_max, B_min, search, what, **goal)     # noqa: E731
    # goal 0; a lambda that no key exceeds gives the table of the fixed-threshold entry at +inf
    for lam in sorted({0, bounds[len(bounds) // 2], max(int(e.max()) - 1, 0)}):
        go(lam=lam)
    for lam in (int(e.max()), (1 << 32) - 1):
        leaves, _, stats = go(lam=lam)
        assert (leaves == tables[B_max]).all() and int(stats[0]) == s_top
    # goal 1: at most M leaves, and one lambda less would be too many
    for M in sorted({n_top, n_top + 3, (n_top + n_max) // 2, n_max - 1, n_max + 10}):
        leaves, lam, stats = go(max_leaves=M)
        assert n_top <= len(leaves) <= M
        if lam > 0:
            assert len(E.rd(B_max, B_min, search, lam=lam - 1)[0]) > M, f"{what}: M = {M}: lambda {lam} - 1 does not overshoot"
        if search == "reference":                               # the threshold rule at the same size is never better
            _, t, bstats = E.budget(B_max, B_min, len(leaves))
            print(f"{what}: M = {M}: RD {len(leaves)} leaves SSE {int(stats[0])}; threshold budget {int(bstats[1:].sum())} leaves SSE {int(bstats[0])}")
            assert int(bstats[0]) >= int(stats[0]), f"{what}: the threshold budget of {len(leaves)} leaves beats the pruning"
    # goal 2: the fewest leaves with D <= max_sse; the next boundary above misses it
    d0 = rd.tree_nd(sse, B_max, B_min, 0)[1]
    for target in sorted({d0, (d0 + s_top) // 2, s_top - 1, s_top, s_top + 5, (1 << 64) - 1}):
        if target < d0:
            continue
        leaves, lam, stats = go(max_sse=target)
        assert int(stats[0]) <= target and lam in bounds
        i = bounds.index(lam)
        if i + 1 < len(bounds):
            assert int(E.rd(B_max, B_min, search, lam=bounds[i + 1])[2][0]) > target, f"{what}: max_sse = {target}: a smaller tree meets it too"
        else:
            assert len(leaves) == n_top
    for target in sorted({0, d0 - 1} - {-1}):                   # out of reach: T(0), and the statistics say so
        if target < d0:
            leaves, lam, stats = go(max_sse=target)
            assert lam == 0 and int(stats[0]) == d0 > target
    # the streams: the leaf tables as they are
    leaves, lam, _ = go(max_leaves=(n_top + n_max) // 2)
    run, got, model = E.stream(leaves, B_max, B_min)
    assert len(run) == 32 + 4 * (E.cols - (2 if E.codec != "grey-iso1" else 3)) * len(leaves)
    assert got[0].shape[:2] == (h, w) and 1 <= got[2] <= 50
    if decode_model:
        ref = model(run)
        assert (got[0] == ref[0]).all() and gc_same(got[1], ref[1]) and int(got[2]) == ref[2], f"{what}: the decode of the RD stream"


def gc_same(a, b):
    return int(np.float32(a).view(np.uint32)) == int(np.float32(b).view(np.uint32))


CODECS = ("grey-iso1", "grey-iso8", "rgb", "rgbiso-iso8")
GEOMETRIES = [   # w, h, wK, ladders, compare the decode with the model's
    (32, 32, 1, LEVELS, False),                 # 4 top-level blocks: one wave, partly filled
    (64, 48, 2, [(16, 4)], False),              # not square, a window
    (64, 64, 0, [(16, 4), (16, 8)], True),      # full search
]


@pytest.mark.parametrize("search", ["reference", "lsq"])
@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("w,h,wK,ladders,decode_model", GEOMETRIES, ids=[f"{g[0]}x{g[1]}-wK{g[2]}" for g in GEOMETRIES])
def test_rd_entries_match_the_model(w, h, wK, ladders, decode_model, codec, search):
    c = gc.QtCase(w, h, 16, 4, wK, "S", 9100 + 5 * w + h + wK)
    E = _Codec(codec, gc.qt_image(c), w, h, wK)
    for B_max, B_min in ladders:
        _check_all_goals(E, B_max, B_min, search, f"{w}x{h} wK={wK} {codec} {search} {B_max}->{B_min}", decode_model and (B_max, B_min) == (16, 4))


def test_grey_argb_twin_and_short_buffer():
    """The ARGB entry gives the bytes of the u8 entry; a short leaf buffer is FIC_E_CAPACITY with the count and lambda set."""
    import ctypes as C
    c = gc.QtCase(64, 64, 16, 4, 0, "S", 9433)
    E = _Codec("grey-iso1", gc.qt_image(c), 64, 64, 0)
    grey_argb = np.ascontiguousarray(fic_amd.RasterImage.from_gray(E.g).argb.reshape(64, 64), np.int32)
    for search in ("reference", "lsq"):
        for goal in ({"lam": 300}, {"max_leaves": 100}, {"max_sse": 2_000_000}):
            a = fic_amd.encode_gray_quadtree_rd(E.g, 16, 4, 0, 1, search=search, **goal)
            b = fic_amd.encode_gray_quadtree_rd(grey_argb, 16, 4, 0, 1, search=search, **goal)
            assert (a[0] == b[0]).all() and a[1] == b[1] and (a[2] == b[2]).all()
    want, lam_want, _ = fic_amd.encode_gray_quadtree_rd(E.g, 16, 4, 0, 1, max_leaves=100)
    assert len(want) <= 100
    out = np.zeros((256, 7), np.int32)
    n, lam = C.c_int(-1), C.c_uint32(0)
    args = (capi.ptr(E.g, C.c_uint8), 64, 64, 16, 4, 0, 1, 0, 1, 100, 0, capi.ptr(out, C.c_int32))
    assert capi.lib().fic_encode_gray_quadtree_rd_u8(*args, len(want) - 1, C.byref(n), C.byref(lam), None) == -8
    assert n.value == len(want) and lam.value == lam_want and not out.any()
    assert capi.lib().fic_encode_gray_quadtree_rd_u8(*args, 256, C.byref(n), C.byref(lam), None) == 0          # stats4 may be NULL
    assert n.value == len(want) and (out[:n.value] == want).all()
    by_bytes = fic_amd.encode_gray_quadtree_rd(E.g, 16, 4, 0, 1, max_bytes=32 + 16 * 100 + 7)
    assert (by_bytes[0] == want).all() and by_bytes[1] == lam_want


# ---- the full image, once per codec -----------------------------------------------------------------------------------------------
def _lena():
    return np.load(os.path.join(gc.GOLDEN, "lena_grey_256.npy"))


def test_lena256_grey_pinned_rows():
    """The rows of the design's table on the device: LenaGrey 256 x 256, 16 -> 4, full search, 1 isometry, reference criterion."""
    g = _lena()
    E = _Codec("grey-iso1", fic_amd.RasterImage.from_gray(g).argb, 256, 256, 0)
    tables = E.level_tables(16, 4, "reference")
    sse = E.sse(16, 4, "reference", tables)
    for M, lam_want, n_want, d_want in ((259, 88438, 259, 24014853), (1024, 5226, 1024, 8726643), (4095, 0, 3799, 6141062)):
        leaves, lam, stats = _check_rd(E, sse, tables, 16, 4, "reference", "lena256", max_leaves=M)
        assert (lam, len(leaves), int(stats[0])) == (lam_want, n_want, d_want)
        assert int(E.budget(16, 4, len(leaves))[2][0]) >= d_want
    leaves, lam, stats = _check_rd(E, sse, tables, 16, 4, "reference", "lena256", max_sse=8726643)
    assert int(stats[0]) <= 8726643 and len(leaves) <= 1024
    _check_rd(E, sse, tables, 16, 4, "reference", "lena256", max_sse=8726642)
    run, got, model = E.stream(leaves, 16, 4)
    assert len(run) == 32 + 16 * 1024 and got[0].shape == (256, 256)


@pytest.mark.parametrize("codec,search", [("rgb", "reference"), ("rgbiso-iso8", "lsq"), ("grey-iso8", "lsq")])
def test_lena256_other_codecs(lena_colored, codec, search):
    from oracle import fic_oracle as fo
    E = _Codec(codec, fo.rgb_to_argb(np.ascontiguousarray(lena_colored)), 256, 256, 0)
    tables = E.level_tables(16, 4, search)
    sse = E.sse(16, 4, search, tables)
    leaves, lam, stats = _check_rd(E, sse, tables, 16, 4, search, f"lena256 {codec} {search}", max_leaves=1024)
    assert lam > 0 and len(leaves) <= 1024 and len(E.rd(16, 4, search, lam=lam - 1)[0]) > 1024
    _check_rd(E, sse, tables, 16, 4, search, f"lena256 {codec} {search}", max_sse=int(stats[0]) + 1000)
    if search == "reference":
        assert int(E.budget(16, 4, len(leaves))[2][0]) >= int(stats[0])
    run, got, _ = E.stream(leaves, 16, 4)
    assert got[0].shape[:2] == (256, 256)


def test_many_workgroups_1024():
    """Lena enlarged to 1024 x 1024, 16 -> 4: 4096 + 16384 keys over many workgroups in the key kernel, both selects and the walkers."""
    g = synth.enlarge(_lena(), 1024, 1024)
    sse = {B: v.astype(np.int64) for B, v in capi.debug_quadtree_sse(g, 16, 4, 0, 1).items()}
    e, G = rd.keys_gains(sse, 16, 4)
    assert e.size == 20480
    s_top = int(sse[16].sum())
    for goal, kind, value in ((rd.GOAL_LEAVES, "max_leaves", 20000), (rd.GOAL_SSE, "max_sse", rd.d_of(e, G, s_top, int(np.median(e))) + 17)):
        lam_want = rd.choose(sse, 1024, 1024, 16, 4, goal, value)
        leaves, lam, stats = fic_amd.encode_gray_quadtree_rd(g, 16, 4, 0, 1, **{kind: value})
        assert lam == lam_want > 0
        assert (len(leaves), int(stats[0])) == rd.tree_nd(sse, 16, 4, lam) == (rd.n_of(e, 4096, lam), rd.d_of(e, G, s_top, lam))
        assert [tuple(r) for r in leaves[:, :3]] == rd.tree(sse, 1024, 1024, 16, 4, lam)
