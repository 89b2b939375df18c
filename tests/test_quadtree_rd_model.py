"""Quadtree encode by rate-distortion pruning, CPU side: the numpy model of the rule
(tests/qtrdmodel.py: cost J, wants-to-split, k(v) by its defining property) on the oracle's level SSEs of LenaGrey 256 x 256 and
of its 64 x 64 crop and on SSE arrays that no encode produces: the identities N = N_top + 3 #{e > lam} and D = sum S_top -
sum_{e > lam} G against the trees built from the rule, monotonicity, optimality against a knapsack over the top-level blocks,
the pinned rows of the design's table, the choice of lam for a leaf budget and for an SSE target, and what the library refuses
without a device."""
import ctypes as C

import numpy as np
import pytest

import qtbudgetmodel as qb
import qtmodel as qm
import qtrdmodel as rd

import fic_amd
from fic_amd import capi

LEVELS = [(16, 4), (8, 4), (16, 8)]


@pytest.fixture(scope="module")
def sse_of(lena_grey, oracle):
    """{name: (w, h, {B: SSE [Rh, Rw]})}: LenaGrey 256 x 256 and its top-left 64 x 64 crop, 16 -> 4, full search, 1 isometry,
    reference criterion.  The levels of a shorter ladder are encoded alone, so 8 -> 4 and 16 -> 8 read the same arrays."""
    out = {}
    for name, g in (("lena256", lena_grey), ("crop64", np.ascontiguousarray(lena_grey[:64, :64]))):
        out[name] = (g.shape[1], g.shape[0], qm.level_sse(g, qm.codebooks(g, 16, 4, 0, 1)))
    return out


def _lams(e):
    """Every key value, its predecessor, 0 and 2^31, ascending."""
    ks = set(int(k) for k in e)
    return sorted({0, 1 << 31} | ks | {k - 1 for k in ks if k > 0})


def _check_rule(sse, w, h, B_max, B_min, what):
    """The identities, the property that defines k, monotonicity and optimality on one set of SSE arrays."""
    n_top, s_top = (w // B_max) * (h // B_max), int(np.asarray(sse[B_max]).astype(np.int64).sum())
    e, G = rd.keys_gains(sse, B_max, B_min)
    assert e.size == G.size == sum(np.asarray(sse[B]).size for B in qm.levels(B_max, B_min)[:-1])
    assert e.min() >= 0 and e.max() < 1 << 31
    # k by its property, on the blocks whose key is their own (the top level; e of a child may be its parent's)
    for B in qm.levels(B_max, B_min)[:-1]:
        k = rd.k_of(sse, B, B_min)
        assert not rd.wants(sse, B, B_min, k).any(), what
        assert (rd.wants(sse, B, B_min, np.maximum(k - 1, 0)) | (k == 0)).all(), what
    best = rd.knapsack(sse, B_max, B_min)
    prev = None
    for lam in _lams(e):
        n, d = rd.tree_nd(sse, B_max, B_min, lam)
        assert (n, d) == (rd.n_of(e, n_top, lam), rd.d_of(e, G, s_top, lam)), f"{what}: lam = {lam}"
        assert d == best[(n - n_top) // 3], f"{what}: lam = {lam}: {n} leaves, SSE {d}, the best tree of that size has {best[(n - n_top) // 3]}"
        if prev is not None:
            assert n <= prev[0] and d >= prev[1], f"{what}: lam = {lam}: ({n}, {d}) after {prev}"
        prev = (n, d)
    assert prev == (n_top, s_top)                               # at 2^31 nothing splits
    return e, G


@pytest.mark.parametrize("B_max,B_min", LEVELS)
@pytest.mark.parametrize("name", ["lena256", "crop64"])
def test_identities_monotonicity_and_optimality(sse_of, name, B_max, B_min):
    w, h, sse = sse_of[name]
    _check_rule(sse, w, h, B_max, B_min, f"{name} {B_max}->{B_min}")


@pytest.mark.parametrize("B_max,B_min", LEVELS)
def test_adversarial_sse_arrays(B_max, B_min):
    for name, sse in rd.adversarial(32, 32, B_max, B_min).items():
        e, G = _check_rule(sse, 32, 32, B_max, B_min, f"{name} {B_max}->{B_min}")
        if name in ("equal", "zeros", "all-ones", "one", "children-worse"):
            assert not e.any(), name                            # a split never pays: four children cost at least the parent
        if name == "children-worse":
            assert (G < 0).all()
        if name == "children-free":
            assert e.max() == -(-rd.LAM_MAX // 3) and (e[:(32 // B_max) ** 2] == e.max()).all()
        if name == "one-huge-block":
            assert (e > 0).sum() >= 1 and e[(32 // B_max) ** 2 - 1] > 0


def test_the_tree_in_stream_order(sse_of):
    """tree() lists the leaves of tree_nd()'s tree in the order of the fixed-threshold split; a lam that nothing survives gives
    the top-level blocks, and with the threshold rule's own choice of blocks the two walks agree."""
    w, h, sse = sse_of["crop64"]
    for B_max, B_min in LEVELS:
        e, _ = rd.keys_gains(sse, B_max, B_min)
        for lam in (0, int(np.median(e)), int(e.max()) - 1, int(e.max())):
            t = rd.tree(sse, w, h, B_max, B_min, lam)
            n, d = rd.tree_nd(sse, B_max, B_min, lam)
            assert len(t) == n and sum(int(sse[B][y // B, x // B]) for x, y, B in t) == d
            assert sum(B * B for _, _, B in t) == w * h and len(set(t)) == n
        assert rd.tree(sse, w, h, B_max, B_min, int(e.max())) == qm.split(sse, w, h, B_max, B_min, np.inf)


# max_leaves -> (lam, leaves, collage SSE) of the pruning and (leaves, collage SSE) of the threshold budget: LenaGrey 256, 16 -> 4
PINNED = [
    (259, 88438, 259, 24014853, 259, 24082566), (512, 20115, 511, 14098445, 511, 16378021), (1024, 5226, 1024, 8726643, 1024, 10529619),
    (2048, 617, 2047, 6484663, 2044, 7105832), (4095, 0, 3799, 6141062, 4093, 6599865),
]


@pytest.mark.parametrize("M,lam_want,n_want,d_want,n_thr,d_thr", PINNED)
def test_pinned_rows(sse_of, M, lam_want, n_want, d_want, n_thr, d_thr):
    w, h, sse = sse_of["lena256"]
    lam = rd.choose(sse, w, h, 16, 4, rd.GOAL_LEAVES, M)
    n, d = rd.tree_nd(sse, 16, 4, lam)
    t, _ = qb.budget_threshold(sse, w, h, 16, 4, M)
    thr = qm.split(sse, w, h, 16, 4, t)
    d_t = sum(int(sse[B][y // B, x // B]) for x, y, B in thr)
    print(M, lam, n, d, len(thr), d_t)
    assert (lam, n, d) == (lam_want, n_want, d_want) and (len(thr), d_t) == (n_thr, d_thr)
    assert d <= d_t or n < len(thr)


@pytest.mark.parametrize("B_max,B_min", LEVELS)
@pytest.mark.parametrize("name", ["lena256", "crop64"])
def test_goals(sse_of, name, B_max, B_min):
    w, h, sse = sse_of[name]
    n_top, n_max, s_top = (w // B_max) * (h // B_max), (w // B_min) * (h // B_min), int(sse[B_max].sum())
    e, G = rd.keys_gains(sse, B_max, B_min)
    for M in (n_top, n_top + 2, n_top + 3, (n_top + n_max) // 2, n_max - 1, n_max, n_max + 10):
        lam = rd.lambda_for_leaves(e, n_top, M)
        assert rd.tree_nd(sse, B_max, B_min, lam)[0] <= M
        assert lam == 0 or rd.tree_nd(sse, B_max, B_min, lam - 1)[0] > M
    with pytest.raises(ValueError):
        rd.lambda_for_leaves(e, n_top, n_top - 1)
    bounds = sorted(set(e.tolist()) | {0})
    d0 = rd.tree_nd(sse, B_max, B_min, 0)[1]
    for target in (s_top + 5, s_top, s_top - 1, (s_top + d0) // 2, d0 + 1, d0):
        lam = rd.lambda_for_sse(e, G, s_top, target)
        n, d = rd.tree_nd(sse, B_max, B_min, lam)
        assert d <= target and lam in bounds
        i = bounds.index(lam)
        if i + 1 < len(bounds):                                 # the tree at the next larger boundary misses the target
            assert rd.tree_nd(sse, B_max, B_min, bounds[i + 1])[1] > target
        else:
            assert n == n_top
        assert lam == 0 or rd.tree_nd(sse, B_max, B_min, lam - 1)[0] > n       # the smallest lam of that tree
    assert rd.lambda_for_sse(e, G, s_top, d0 - 1) == 0          # out of reach: T(0)
    assert rd.lambda_for_sse(e, G, s_top, 0) == 0


def test_weighted_select_models_agree():
    rng = np.random.default_rng(7)
    for n in (1, 5, 300):
        keys = rng.integers(0, 40, n)
        gains = rng.integers(0, 100, n)
        total = int(gains.sum())
        for need in [-3, 0, 1, total, total + 1] + rng.integers(0, total + 2, 20).tolist():
            assert rd.select_weighted(keys, gains, need) == rd.select_weighted_fast(keys, gains, need), (n, need)
    assert rd.select_weighted([5, 5, 3], [1, 1, 10], 2) == (3, 2, 2)
    assert rd.select_weighted([5, 5, 3], [1, 1, 10], 3) == (0, 3, 12)
    assert rd.select_weighted([5, 5, 3], [1, 1, 10], 13) == (0, 3, 12)        # out of reach: the last boundary
    assert rd.select_weighted([5, 5, 3], [1, 1, 10], 0) == (5, 0, 0)


# ---- what the library refuses before any device work ------------------------------------------------------------------------------
def _entries(lena64):
    """(name, function, the arguments before `search`, columns) of the four entries on the 64 x 64 image."""
    L = capi.lib()
    g = np.ascontiguousarray(lena64)
    h, w = g.shape
    argb = np.ascontiguousarray(fic_amd.RasterImage.from_gray(g).argb.reshape(h, w), np.int32)
    pg, pa = capi.ptr(g, C.c_uint8), capi.ptr(argb, C.c_int32)
    return [
        ("gray_u8", L.fic_encode_gray_quadtree_rd_u8, [pg, w, h, 16, 4, 0, 1], 7, (g, argb)),
        ("gray_argb", L.fic_encode_gray_quadtree_rd_argb, [pa, w, h, 16, 4, 0, 8], 7, (g, argb)),
        ("rgb", L.fic_encode_rgb_quadtree_rd_argb, [pa, w, h, 16, 4, 0], 8, (g, argb)),
        ("rgb_iso", L.fic_encode_rgb_quadtree_iso_rd_argb, [pa, w, h, 16, 8, 2, 8], 9, (g, argb)),
    ]


def test_library_refuses_bad_arguments_before_the_device(lena64):
    """One refusal per check of the RD entries, with the library loaded and no device needed: -3 FIC_E_ARGUMENT, -1
    FIC_E_GEOMETRY, -2 FIC_E_WINDOW.  An acceptable call then needs the device (-4 without one)."""
    n_top = 16
    for name, fn, head, cols, keep in _entries(lena64):
        out = np.zeros((256, cols), np.int32)
        o, n, lam = capi.ptr(out, C.c_int32), C.c_int(-1), C.c_uint32(77)
        stats = np.zeros(4, np.uint64)

        def call(head=head, search=0, goal=1, value=100, leaves=o, n_p=C.byref(n), lam_p=C.byref(lam), device=0):
            return fn(*head, search, goal, value, device, leaves, 256, n_p, lam_p, capi.ptr(stats, C.c_uint64))

        def with_(i, v):
            h2 = list(head)
            h2[i] = v
            return h2

        assert call(head=with_(0, None)) == -3, name             # null image
        assert call(leaves=None) == -3 and call(n_p=None) == -3 and call(lam_p=None) == -3, name
        assert call(goal=-1) == -3 and call(goal=3) == -3, name
        assert call(search=-1) == -3 and call(search=2) == -3, name
        assert call(goal=0, value=1 << 32) == -3 and call(goal=0, value=(1 << 64) - 1) == -3, name
        assert "lambda" in capi.last_error()
        assert call(goal=1, value=n_top - 1) == -3 and "max_leaves" in capi.last_error(), name
        assert call(goal=1, value=0) == -3, name
        assert call(head=with_(4, 16)) == -3 and call(head=with_(3, 32)) == -3, name      # the ladder: B_min = B_max, B_max = 32
        assert call(head=with_(1, 72)) == -1, name               # 72 is no multiple of 16
        assert call(head=with_(5, -1)) == -2, name               # the window
        if len(head) == 7:
            assert call(head=with_(6, 3)) == -3, name            # n_iso
        assert (n.value, lam.value) == (-1, 77) and not out.any() and not stats.any(), name
        if capi.lib().fic_device_count() < 1:
            for goal, value in ((0, 0), (0, (1 << 32) - 1), (1, n_top), (2, 0), (2, (1 << 64) - 1)):
                assert call(goal=goal, value=value) == -4, (name, goal, value)
            assert call(device=-1) == -4
    # wK = 0 needs a square image
    L = capi.lib()
    g = np.zeros((32, 64), np.uint8)
    out = np.zeros((128, 7), np.int32)
    n, lam = C.c_int(), C.c_uint32()
    assert L.fic_encode_gray_quadtree_rd_u8(capi.ptr(g, C.c_uint8), 64, 32, 16, 4, 0, 1, 0, 0, 0, 0, capi.ptr(out, C.c_int32), 128, C.byref(n),
                                            C.byref(lam), None) == -2


def test_python_entries_take_exactly_one_goal(lena64):
    argb = fic_amd.RasterImage.from_gray(lena64).argb.reshape(64, 64)
    calls = [
        lambda **kw: fic_amd.encode_gray_quadtree_rd(lena64, 16, 4, 0, 1, **kw),
        lambda **kw: fic_amd.encode_rgb_quadtree_rd(argb, 64, 64, 16, 4, 0, **kw),
        lambda **kw: fic_amd.encode_rgb_quadtree_iso_rd(argb, 64, 64, 16, 4, 0, 8, **kw),
    ]
    for call in calls:
        for kw in ({}, {"lam": 1, "max_leaves": 100}, {"max_bytes": 1000, "max_sse": 5}, {"lam": 0, "max_leaves": 20, "max_bytes": 1000, "max_sse": 5}):
            with pytest.raises(ValueError):
                call(**kw)
        for kw in ({"lam": 1 << 32}, {"lam": -1}, {"max_leaves": 15}, {"max_sse": -1}, {"lam": 0, "search": "best"}, {"max_bytes": 32 + 16 * 4}):
            with pytest.raises(fic_amd.FicError) as e:
                call(**kw)
            assert e.value.code == -3, kw
        with pytest.raises(fic_amd.FicError) as e:
            call(max_bytes=31)
        assert e.value.code == -8


def test_hooks_refuse_bad_arguments_before_the_device():
    L = capi.lib()
    sse = np.zeros(4 + 16 + 64, np.uint32)
    keys, gains = np.zeros(20, np.uint32), np.zeros(20, np.int64)
    ps, pk, pg = capi.ptr(sse, C.c_uint32), capi.ptr(keys, C.c_uint32), capi.ptr(gains, C.c_int64)
    assert L.fic_debug_qt_rd_keys(0, None, 32, 32, 16, 4, pk, pg) == -3
    assert L.fic_debug_qt_rd_keys(0, ps, 32, 32, 16, 4, None, pg) == -3
    assert L.fic_debug_qt_rd_keys(0, ps, 32, 32, 16, 4, pk, None) == -3
    assert L.fic_debug_qt_rd_keys(0, ps, 32, 32, 16, 16, pk, pg) == -3
    assert L.fic_debug_qt_rd_keys(0, ps, 40, 32, 16, 4, pk, pg) == -1
    key, above, gain = C.c_uint32(), C.c_int64(), C.c_int64()
    res = (C.byref(key), C.byref(above), C.byref(gain))
    assert L.fic_debug_qt_select_weighted(0, None, pg, 20, 1, *res) == -3
    assert L.fic_debug_qt_select_weighted(0, pk, None, 20, 1, *res) == -3
    assert L.fic_debug_qt_select_weighted(0, pk, pg, 0, 1, *res) == -3
    assert L.fic_debug_qt_select_weighted(0, pk, pg, 20, 1, None, C.byref(above), C.byref(gain)) == -3
    assert L.fic_debug_qt_select_weighted(0, pk, pg, 20, 1, C.byref(key), None, C.byref(gain)) == -3
    assert L.fic_debug_qt_select_weighted(0, pk, pg, 20, 1, C.byref(key), C.byref(above), None) == -3
    if L.fic_device_count() < 1:
        assert L.fic_debug_qt_rd_keys(0, ps, 32, 32, 16, 4, pk, pg) == -4
        assert L.fic_debug_qt_select_weighted(0, pk, pg, 20, 1, *res) == -4
