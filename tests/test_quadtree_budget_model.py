"""Quadtree encode to a leaf budget, CPU side: the numpy model of the threshold rule
(tests/qtbudgetmodel.py) against the split of the quadtree model (qtmodel.split) on the oracle's level codebooks, the pinned
thresholds that the GPU tests rely on, the round-up of keys that no float32 holds, ties, and what the library decides without
a device: the refusal of a budget below N_top and the leaf count of a byte budget."""
import ctypes as C

import numpy as np
import pytest

import isostreammodel as im
import qtbudgetmodel as qb
import qtmodel as qm
import qtrgbmodel as qr

import fic_amd
from fic_amd import capi

LEVELS = [(16, 4), (8, 4), (16, 8)]


@pytest.fixture(scope="module")
def sse_of(lena_grey, oracle):
    """{name: (w, h, {B: SSE [Rh, Rw]})} for LenaGrey 256 x 256 and its top-left 64 x 64 crop, 16 -> 4, full search, 1 isometry.
    The levels of a shorter ladder are encoded alone, so 8 -> 4 and 16 -> 8 read the same arrays."""
    out = {}
    for name, g in (("lena256", lena_grey), ("crop64", np.ascontiguousarray(lena_grey[:64, :64]))):
        out[name] = (g.shape[1], g.shape[0], qm.level_sse(g, qm.codebooks(g, 16, 4, 0, 1)))
    return out


def _below(t):
    return np.nextafter(np.float32(t), np.float32(-np.inf))


def _budgets(w, h, B_max, B_min):
    n_top, n_max = (w // B_max) * (h // B_max), (w // B_min) * (h // B_min)
    return n_top, [n_top, n_top + 2, n_top + 3, (n_top + n_max) // 2, n_max - 1, n_max, n_max + 10]


@pytest.mark.parametrize("B_max,B_min", LEVELS)
@pytest.mark.parametrize("name", ["lena256", "crop64"])
def test_threshold_is_the_smallest_that_meets_the_budget(sse_of, name, B_max, B_min):
    w, h, sse = sse_of[name]
    n_top, budgets = _budgets(w, h, B_max, B_min)
    e = qb.keys(sse, B_max, B_min)
    assert e.size == sum(sse[B].size for B in qm.levels(B_max, B_min)[:-1]) and e.max() < 1 << 24
    for M in budgets:
        t, K = qb.budget_threshold(sse, w, h, B_max, B_min, M)
        assert t.dtype == np.float32 and t >= 0 and float(t) * 256.0 == K           # exact below 2^24
        n = len(qm.split(sse, w, h, B_max, B_min, t))
        assert n <= M, (name, M, t, n)
        assert n == qb.leaves_at(sse, B_max, B_min, t) == n_top + 3 * int((e > K).sum())
        if t > 0:
            assert len(qm.split(sse, w, h, B_max, B_min, _below(t))) > M, (name, M, t)
        else:                                                                       # everything that can split does
            assert n == n_top + 3 * int((e > 0).sum())
    with pytest.raises(ValueError):
        qb.budget_threshold(sse, w, h, B_max, B_min, n_top - 1)


# (image, M) -> (threshold, leaves) at 16 -> 4; the first row is the calibration of test_quadtree_model (threshold 400 <-> 937)
PINNED = [
    ("lena256", 937, 399.078125, 937), ("lena256", 259, 2216.00390625, 259), ("lena256", 4095, 2.4375, 4093),
    ("lena256", 4096, 0.0, 4096), ("lena256", 5000, 0.0, 4096), ("crop64", 46, 119.109375, 46), ("crop64", 255, 6.1875, 253),
]


@pytest.mark.parametrize("name,M,t_want,n_want", PINNED)
def test_pinned_thresholds(sse_of, name, M, t_want, n_want):
    w, h, sse = sse_of[name]
    t, K = qb.budget_threshold(sse, w, h, 16, 4, M)
    n = len(qm.split(sse, w, h, 16, 4, t))
    print(name, M, repr(float(t)), K, n)
    assert (float(t), n) == (t_want, n_want)
    if (name, M) == ("lena256", 937):
        assert K == 102164 and n == len(qm.split(sse, w, h, 16, 4, 400.0))


def test_keys_that_no_float_holds_round_up():
    """Keys in [2^24, 2^26) that are no multiple of 4 (colour SSE at B = 16): the threshold is the float above K / 256, the
    block of key K stays whole under it and splits under the float below."""
    rng = np.random.default_rng(20261019)
    for K in [(1 << 24) + 1, (1 << 25) + 1, (1 << 25) + 2, (1 << 25) + 3, (1 << 26) - 1] + [int(v) | 1 for v in rng.integers(1 << 24, 1 << 26, 50)]:
        t = qb.key_threshold(K)
        assert t.dtype == np.float32 and float(t) * 256.0 > K > float(_below(t)) * 256.0
    for K in (0, 1, 255, (1 << 24) - 1, 1 << 24, (1 << 24) + 2, (1 << 25) + 4, 1 << 25):
        assert float(qb.key_threshold(K)) * 256.0 == K
    assert qb.key_threshold((1 << 32) - 1) == np.float32(2.0 ** 24)
    # through the whole rule: a 64 x 64 colour-like image of 16 blocks at 16 -> 8, every SSE odd and above 2^24
    s16 = (rng.integers(1 << 24, 1 << 26, (4, 4)) | 1).astype(np.int64)
    sse = {16: s16, 8: np.zeros((8, 8), np.int64)}
    order = np.sort(s16.reshape(-1))[::-1]
    for S in (0, 1, 7, 15):
        M = 16 + 3 * S + 1
        t, K = qb.budget_threshold(sse, 64, 64, 16, 8, M)
        assert K == order[S] and float(t) * 256.0 > K
        n = len(qm.split(sse, 64, 64, 16, 8, t))
        assert n <= M and len(qm.split(sse, 64, 64, 16, 8, _below(t))) > M
        assert n == 16 + 3 * int((s16.astype(np.float64) > 256.0 * float(t)).sum())     # a neighbour of K may stay whole too
    assert qb.budget_threshold(sse, 64, 64, 16, 8, 64)[0] == 0


def test_a_child_never_counts_before_its_parent():
    """e(v) = min over the ancestors: a level-1 block of large SSE under a parent of small SSE takes the parent's key."""
    sse = {16: np.array([[10, 300], [0, 50]]), 8: np.full((4, 4), 1000), 4: np.zeros((8, 8), np.int64)}
    e = qb.keys(sse, 16, 4)
    assert e[:4].tolist() == [10, 300, 0, 50] and sorted(set(e[4:].tolist())) == [0, 10, 50, 300]
    for M in range(4, 70):
        t, K = qb.budget_threshold(sse, 32, 32, 16, 4, M)
        n = len(qm.split(sse, 32, 32, 16, 4, t))
        assert n <= M and n == qb.leaves_at(sse, 16, 4, t)
        assert t == 0 or len(qm.split(sse, 32, 32, 16, 4, _below(t))) > M


def test_ties_are_not_broken(oracle):
    """An image of one repeated tile: every top-level block has the same key, so a budget with room for one split gets none."""
    tile = np.random.default_rng(5).integers(0, 256, (16, 16), dtype=np.uint8)
    g = np.ascontiguousarray(np.tile(tile, (4, 4)))
    sse = qm.level_sse(g, qm.codebooks(g, 16, 8, 0, 1))
    assert len(set(sse[16].reshape(-1).tolist())) == 1 and sse[16][0, 0] > 0
    t, K = qb.budget_threshold(sse, 64, 64, 16, 8, 16 + 3)
    assert K == sse[16][0, 0] and len(qm.split(sse, 64, 64, 16, 8, t)) == 16
    assert len(qm.split(sse, 64, 64, 16, 8, _below(t))) == 64


def test_library_refuses_a_budget_below_n_top_before_the_device(lena64):
    """N_top - 1 leaves: FIC_E_ARGUMENT from every budget entry, with or without a device; N_top passes the check (and then
    needs the device)."""
    h, w = lena64.shape
    argb = fic_amd.RasterImage.from_gray(lena64).argb.reshape(h, w)
    n_top = (w // 16) * (h // 16)
    calls = [
        lambda M: capi.encode_gray_quadtree_budget(lena64, 16, 4, 0, 1, max_leaves=M),
        lambda M: capi.encode_gray_quadtree_budget(argb, 16, 4, 0, 8, max_leaves=M),
        lambda M: capi.encode_rgb_quadtree_budget(argb, w, h, 16, 4, 0, max_leaves=M),
        lambda M: capi.encode_rgb_quadtree_iso_budget(argb, w, h, 16, 8, 2, 8, max_leaves=M),
    ]
    for call in calls:
        for M in (n_top - 1, 0, -5):
            with pytest.raises(fic_amd.FicError) as e:
                call(M)
            assert e.value.code == -3 and "max_leaves" in str(e.value)
        if capi.lib().fic_device_count() < 1:
            with pytest.raises(fic_amd.FicError) as e:
                call(n_top)
            assert e.value.code == -4
        for kw in ({}, {"max_leaves": 100, "max_bytes": 1000}):
            with pytest.raises(ValueError):
                capi.encode_gray_quadtree_budget(lena64, 16, 4, **kw)
    # null pointers, and the other argument checks keep their codes
    L, n, t = capi.lib(), C.c_int(), C.c_float()
    out = np.zeros((256, 7), np.int32)
    g = np.ascontiguousarray(lena64)
    head = (capi.ptr(g, C.c_uint8), w, h, 16, 4, 0, 1, 100, 0)
    assert L.fic_encode_gray_quadtree_budget_u8(*head, capi.ptr(out, C.c_int32), 256, C.byref(n), None, None) == -3
    assert L.fic_encode_gray_quadtree_budget_u8(*head, None, 256, C.byref(n), C.byref(t), None) == -3
    assert L.fic_encode_gray_quadtree_budget_u8(None, *head[1:], capi.ptr(out, C.c_int32), 256, C.byref(n), C.byref(t), None) == -3
    with pytest.raises(fic_amd.FicError) as e:
        capi.encode_gray_quadtree_budget(lena64, 16, 16, max_leaves=100)
    assert e.value.code == -3
    with pytest.raises(fic_amd.FicError) as e:
        capi.encode_gray_quadtree_budget(np.zeros((72, 72), np.uint8), 16, 4, max_leaves=100)
    assert e.value.code == -1
    key, above = C.c_uint32(), C.c_int64()
    k = np.zeros(4, np.uint32)
    assert L.fic_debug_qt_select(0, None, 4, 0, C.byref(key), C.byref(t), C.byref(above)) == -3
    assert L.fic_debug_qt_select(0, capi.ptr(k, C.c_uint32), 0, 0, C.byref(key), C.byref(t), C.byref(above)) == -3
    assert L.fic_debug_qt_select(0, capi.ptr(k, C.c_uint32), 4, -1, C.byref(key), C.byref(t), C.byref(above)) == -3


def test_leaves_for_bytes_against_the_stream_writers():
    writers = [   # tag, n_iso, ints per leaf, the model's writer of n leaves
        (2, 1, 4, lambda n: qm.write_run(np.zeros((n, 7), np.int32), 64, 64, 16, 4, 0, 1)),
        (2, 8, 5, lambda n: qm.write_run(np.zeros((n, 7), np.int32), 64, 64, 16, 4, 0, 8)),
        (3, 1, 6, lambda n: qr.write_run(np.zeros((n, 8), np.int32), 64, 64, 16, 4, 0)),
        (6, 1, 7, lambda n: im.write_qt(np.zeros((n, 9), np.int32), 64, 64, 16, 4, 0)),
        (6, 8, 7, lambda n: im.write_qt(np.zeros((n, 9), np.int32), 64, 64, 16, 4, 0)),
    ]
    for tag, n_iso, ints, write in writers:
        for n in (0, 1, 2, 16, 937, 65536):
            size = len(write(n))
            assert size == 32 + 4 * ints * n
            assert capi.quadtree_leaves_for_bytes(tag, n_iso, size) == n
            assert capi.quadtree_leaves_for_bytes(tag, n_iso, size + 4 * ints - 1) == n
            assert capi.quadtree_leaves_for_bytes(tag, n_iso, size + 4 * ints) == n + 1
        assert capi.quadtree_leaves_for_bytes(tag, n_iso, (1 << 40) + 32) == (1 << 40) // (4 * ints)
        with pytest.raises(fic_amd.FicError) as e:
            capi.quadtree_leaves_for_bytes(tag, n_iso, 31)
        assert e.value.code == -8
    for tag, n_iso in ((0, 1), (1, 1), (4, 1), (5, 8), (7, 1), (2, 3), (6, 0), (3, 8)):
        with pytest.raises(fic_amd.FicError) as e:
            capi.quadtree_leaves_for_bytes(tag, n_iso, 1000)
        assert e.value.code == -3
