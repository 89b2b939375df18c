"""Quadtree encode to a leaf budget on the GPU against the numpy model (tests/qtbudgetmodel.py):
the radix select alone on hand-made key sets against numpy's sort, and the budget entries of every quadtree format against
the model's threshold on the library's own per-level SSE, against the fixed-threshold entry at that threshold (leaf table bit
for bit), against the float just below it (which must overshoot), and against the sums of the leaf table (stats)."""
import ctypes as C
import os

import numpy as np
import pytest

import geomcases as gc
import qtbudgetmodel as qb
import qtmodel as qm
import qtrgbmodel as qr

import fic_amd
from fic_amd import capi, synth

pytestmark = pytest.mark.gpu


def _below(t):
    return np.nextafter(np.float32(t), np.float32(-np.inf))


def _bits(t):
    return int(np.float32(t).view(np.uint32))


# ---- the select alone -----------------------------------------------------------------------------------------------------------
def _key_sets():
    rng = np.random.default_rng(20261019)
    sets = {f"n{n}": rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) for n in (1, 4, 20, 255, 256, 257)}
    sets["n2^20+3"] = rng.integers(0, 1 << 26, (1 << 20) + 3, dtype=np.uint64).astype(np.uint32)   # many workgroups, the grid stride
    sets["equal"] = np.full(257, 0x01020304, np.uint32)
    sets["top-byte"] = (rng.integers(0, 256, 300, dtype=np.uint64) << 24).astype(np.uint32) | np.uint32(0x00ABCDEF)
    sets["bottom-byte"] = rng.integers(0, 256, 300, dtype=np.uint64).astype(np.uint32) | np.uint32(0x12345600)
    sets["zero-and-max"] = np.where(rng.random(259) < 0.5, 0, 0xFFFFFFFF).astype(np.uint32)
    sets["all-zero"] = np.zeros(70, np.uint32)
    sets["all-max"] = np.full(65, 0xFFFFFFFF, np.uint32)
    sets["odd-2^24..2^26"] = (rng.integers(1 << 24, 1 << 26, 300, dtype=np.uint64) | 1).astype(np.uint32)   # colour keys no float holds
    sets["odd-2^24..2^26-large"] = (rng.integers(1 << 24, 1 << 26, 70001, dtype=np.uint64) | 1).astype(np.uint32)
    return sets


KEY_SETS = _key_sets()


@pytest.mark.parametrize("name", list(KEY_SETS))
def test_select_matches_numpy_sort(name):
    keys = KEY_SETS[name]
    n = keys.size
    desc = np.sort(keys)[::-1].astype(np.int64)
    ranks = range(n + 1) if n <= 300 else sorted({0, 1, n - 1, n, n + 5} | set(np.random.default_rng(n).integers(0, n, 20).tolist()))
    for r in ranks:
        K = int(desc[r]) if r < n else 0
        got = capi.debug_qt_select(keys, r)
        want = (K, qb.key_threshold(K), int((desc > K).sum()))
        assert (got[0], _bits(got[1]), got[2]) == (want[0], _bits(want[1]), want[2]), f"{name}: rank {r}: {got}, numpy {want}"
        if name.startswith("odd") and r < n:
            assert float(got[1]) * 256.0 > K > float(_below(got[1])) * 256.0        # the float above K / 256, not the nearest
    assert capi.debug_qt_select(keys, 1 << 40)[0] == 0                              # any rank past the keys


# ---- the budget entries of every format -----------------------------------------------------------------------------------------
class _Grey:
    cols = 7

    def __init__(self, c, n_iso):
        self.c, self.n_iso = c, n_iso
        self.g = np.ascontiguousarray(qr.channels(gc.qt_image(c), c.w, c.h)[..., 0].astype(np.uint8))

    def sse(self):
        return capi.debug_quadtree_sse(self.g, self.c.B_max, self.c.B_min, self.c.wK, self.n_iso)

    def fixed(self, t):
        return capi.encode_gray_quadtree(self.g, self.c.B_max, self.c.B_min, self.c.wK, self.n_iso, t)

    def budget(self, **kw):
        return capi.encode_gray_quadtree_budget(self.g, self.c.B_max, self.c.B_min, self.c.wK, self.n_iso, **kw)


class _Rgb:
    cols = 8

    def __init__(self, c, n_iso):
        self.c, self.n_iso, self.a = c, n_iso, gc.qt_image(c)

    def sse(self):
        return capi.debug_rgb_quadtree_sse(self.a, self.c.w, self.c.h, self.c.B_max, self.c.B_min, self.c.wK)

    def fixed(self, t):
        return capi.encode_rgb_quadtree(self.a, self.c.w, self.c.h, self.c.B_max, self.c.B_min, self.c.wK, t)

    def budget(self, **kw):
        return capi.encode_rgb_quadtree_budget(self.a, self.c.w, self.c.h, self.c.B_max, self.c.B_min, self.c.wK, **kw)


class _RgbIso(_Rgb):
    cols = 9

    def sse(self):
        return capi.debug_rgb_quadtree_iso_sse(self.a, self.c.w, self.c.h, self.c.B_max, self.c.B_min, self.c.wK, self.n_iso)

    def fixed(self, t):
        return capi.encode_rgb_quadtree_iso(self.a, self.c.w, self.c.h, self.c.B_max, self.c.B_min, self.c.wK, self.n_iso, t)

    def budget(self, **kw):
        return capi.encode_rgb_quadtree_iso_budget(self.a, self.c.w, self.c.h, self.c.B_max, self.c.B_min, self.c.wK, self.n_iso, **kw)


def _encoder(c, encoder):
    if encoder.startswith("grey"):
        return _Grey(c, int(encoder[-1]))
    return _Rgb(c, 1) if encoder == "rgb" else _RgbIso(c, int(encoder[-1]))


BUDGET_GEOMETRIES = [(16, 16, 8, 4, 1), (32, 32, 16, 4, 1), (48, 32, 16, 4, 1), (80, 80, 16, 4, 0)]   # 4 keys, 4 + 16, ragged, full search
BUDGET_CASES = [c for c in gc.QT_CASES if (c.w, c.h, c.B_max, c.B_min, c.wK) in BUDGET_GEOMETRIES]
assert len(BUDGET_CASES) == 2 * len(BUDGET_GEOMETRIES) and all(g in gc.QT_GEOMETRIES for g in BUDGET_GEOMETRIES)


def _check_budget(E, sse, w, h, B_max, B_min, M, what):
    n_top = (w // B_max) * (h // B_max)
    t_want, K = qb.budget_threshold(sse, w, h, B_max, B_min, M)
    leaves, t, stats = E.budget(max_leaves=M)
    print(f"{what}: M = {M}: threshold {float(t)!r} (K = {K}), {len(leaves)} leaves, stats {stats.tolist()}")
    assert t.dtype == np.float32 and _bits(t) == _bits(t_want), f"{what}: M = {M}: threshold {float(t)!r}, model {float(t_want)!r} (K = {K})"
    want = E.fixed(t)
    assert leaves.shape == want.shape and (leaves == want).all(), f"{what}: M = {M}: leaves against the fixed-threshold entry at {float(t)!r}"
    assert leaves.shape[1] == E.cols and n_top <= len(leaves) <= M
    assert len(leaves) == qb.leaves_at(sse, B_max, B_min, t) == len(qm.split(sse, w, h, B_max, B_min, t))
    if t > 0:
        assert len(E.fixed(_below(t))) > M, f"{what}: M = {M}: the float below {float(t)!r} does not overshoot"
    else:
        assert len(leaves) == n_top + 3 * int((qb.keys(sse, B_max, B_min) > 0).sum())
    assert (stats == qb.tree_stats(sse, leaves, B_max)).all(), f"{what}: M = {M}: stats {stats.tolist()}"
    assert int(stats[1:].sum()) == len(leaves)
    return leaves, t


@pytest.mark.parametrize("encoder", gc.QT_ENCODERS)
@pytest.mark.parametrize("c", BUDGET_CASES, ids=gc.qt_case_id)
def test_budget_matches_model_and_fixed_threshold(c, encoder):
    E = _encoder(c, encoder)
    sse = {B: v.astype(np.int64) for B, v in E.sse().items()}
    n_top, n_max = (c.w // c.B_max) * (c.h // c.B_max), (c.w // c.B_min) * (c.h // c.B_min)
    for M in (n_top, n_top + 3, (n_top + n_max) // 2, n_max):
        _check_budget(E, sse, c.w, c.h, c.B_max, c.B_min, M, f"{gc.qt_case_id(c)} {encoder}")


def _lena():
    return np.load(os.path.join(gc.GOLDEN, "lena_grey_256.npy"))


def test_lena256_budget_937():
    """The calibration of test_quadtree_model (threshold 400 <-> 937 leaves) the other way round, through to the decoder."""
    g = _lena()
    c = gc.QtCase(256, 256, 16, 4, 0, "lena", 0)
    E = _Grey.__new__(_Grey)
    E.c, E.n_iso, E.g = c, 1, g
    sse = {B: v.astype(np.int64) for B, v in E.sse().items()}
    leaves, t = _check_budget(E, sse, 256, 256, 16, 4, 937, "lena256")
    assert float(t) == 399.078125 and len(leaves) == 937
    assert (leaves == E.fixed(400.0)).all()
    # the ARGB twin
    twin, t2, _ = capi.encode_gray_quadtree_budget(fic_amd.RasterImage.from_gray(g).argb.reshape(256, 256), 16, 4, 0, 1, max_leaves=937)
    assert _bits(t2) == _bits(t) and (twin == leaves).all()
    run = fic_amd.write_run_quadtree(leaves, 256, 256, 16, 4, 0, 1)
    got, want = fic_amd.decode_quadtree_run(run), qm.decode(run)
    assert (got[0] == want[0]).all() and _bits(got[1]) == _bits(want[1]) and got[2] == want[2]


def test_multi_workgroup_select_1024_and_byte_budget():
    """Lena enlarged to 1024 x 1024 at 16 -> 4: 4096 + 16384 keys, histograms over many workgroups; a mid budget, and a byte
    budget through the Python entry."""
    g = synth.enlarge(_lena(), 1024, 1024)
    c = gc.QtCase(1024, 1024, 16, 4, 0, "lena", 0)
    E = _Grey.__new__(_Grey)
    E.c, E.n_iso, E.g = c, 1, g
    sse = {B: v.astype(np.int64) for B, v in E.sse().items()}
    assert qb.keys(sse, 16, 4).size == 20480
    leaves, t = _check_budget(E, sse, 1024, 1024, 16, 4, (4096 + 65536) // 2, "lena1024")
    assert t > 0
    max_bytes = 100000
    M = (max_bytes - 32) // 16
    assert capi.quadtree_leaves_for_bytes(2, 1, max_bytes) == M
    by_bytes, tb, stats = capi.encode_gray_quadtree_budget(g, 16, 4, 0, 1, max_bytes=max_bytes)
    assert _bits(tb) == _bits(qb.budget_threshold(sse, 1024, 1024, 16, 4, M)[0])
    run = fic_amd.write_run_quadtree(by_bytes, 1024, 1024, 16, 4, 0, 1)
    assert len(run) <= max_bytes and len(by_bytes) == qb.leaves_at(sse, 16, 4, tb) and (stats == qb.tree_stats(sse, by_bytes, 16)).all()
    assert len(qm.split(sse, 1024, 1024, 16, 4, _below(tb))) > M


def test_refusals_and_short_buffer():
    g = np.ascontiguousarray(_lena()[:64, :64])
    L = capi.lib()
    p = capi.ptr(g, C.c_uint8)
    out = np.zeros((256, 7), np.int32)
    n, t = C.c_int(-1), C.c_float(-1.0)
    stats = np.zeros(4, np.uint64)
    args = lambda M, leaves, cap, np_, tp: (p, 64, 64, 16, 4, 0, 1, M, 0, leaves, cap, np_, tp, capi.ptr(stats, C.c_uint64))  # noqa: E731
    o = capi.ptr(out, C.c_int32)
    assert L.fic_encode_gray_quadtree_budget_u8(*args(15, o, 256, C.byref(n), C.byref(t))) == -3          # M < N_top = 16
    assert L.fic_encode_gray_quadtree_budget_u8(*args(100, None, 256, C.byref(n), C.byref(t))) == -3
    assert L.fic_encode_gray_quadtree_budget_u8(*args(100, o, 256, None, C.byref(t))) == -3
    assert L.fic_encode_gray_quadtree_budget_u8(*args(100, o, 256, C.byref(n), None)) == -3
    assert (n.value, t.value) == (-1, -1.0)
    want, t_want, _ = capi.encode_gray_quadtree_budget(g, 16, 4, 0, 1, max_leaves=100)
    assert 16 < len(want) <= 100
    # a short leaf buffer: FIC_E_CAPACITY, the count and the threshold still set, nothing written
    assert L.fic_encode_gray_quadtree_budget_u8(*args(100, o, len(want) - 1, C.byref(n), C.byref(t))) == -8
    assert n.value == len(want) and _bits(t.value) == _bits(t_want) and not out.any()
    # stats4 may be NULL
    n, t = C.c_int(-1), C.c_float(-1.0)
    assert L.fic_encode_gray_quadtree_budget_u8(p, 64, 64, 16, 4, 0, 1, 100, 0, o, 256, C.byref(n), C.byref(t), None) == 0
    assert n.value == len(want) and (out[:n.value] == want).all() and _bits(t.value) == _bits(t_want)
