"""Lifetime of device memory under the C ABI (csrc/fic_devmem.h): every path that allocates -- the contexts' first-use stores,
the one-shot caches, the decoders' arenas, one-call scratch -- runs through the counted pair behind fic_debug_live_memory, so a
store that is never freed shows as counters that do not come back to zero.  Every test starts from zero, sees the counters
non-zero while something is alive, and ends at zero, bytes and allocation counts, device and pinned.  Every encode is also
compared bit for bit with a fresh context that ran only that configuration: a store kept from another configuration (another
operand type, fewer slots) must not change a result."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import same_f32  # noqa: E402

import fic_amd  # noqa: E402
from fic_amd import capi  # noqa: E402

pytestmark = pytest.mark.gpu

W = H = 64
ZERO = dict.fromkeys(capi.LIVE_MEMORY_FIELDS, 0)


@pytest.fixture
def counted():
    """Starts from nothing live and ends there."""
    capi.release_cache()
    assert capi.live_memory() == ZERO
    yield
    capi.release_cache()
    assert capi.live_memory() == ZERO


def _alive():
    m = capi.live_memory()
    assert m["device_bytes"] > 0 and m["device_allocations"] > 0, m
    return m


def _same(got, want, what):
    assert got.keys() == want.keys(), what
    for k in got:
        if got[k].dtype == np.float32:
            assert same_f32(got[k], want[k]), f"{what}: bits of {k}"
        else:
            assert (got[k] == want[k]).all(), f"{what}: {k}"


def _argb(gray):
    return fic_amd.RasterImage.from_gray(gray).argb


def _colour():
    rng = np.random.default_rng(3)
    return (rng.integers(0, 1 << 24, W * H).astype(np.uint32) | 0xFF000000).view(np.int32)


# ---- 1. a grey context through every lazy path ----------------------------------------------------------------------------------
def _configure(enc, sweep, search, chunks):
    enc.set_option("search", 0)          # always allowed; then the sweep, which "search" = lsq restricts to 0..2
    enc.set_option("sweep", sweep)
    enc.set_option("search", search)
    enc.set_option("chunks", chunks)


def _grey_results(enc, search):
    r = enc.results()
    if search:
        r["E"] = enc.lsq_error()
    return r


def _fresh_grey(img, B, wK, n_iso, sweep, search, chunks):
    with fic_amd.Encoder(W, H, B, wK, n_iso) as e:
        _configure(e, sweep, search, chunks)
        e.set_gray(img)
        e.encode()
        return _grey_results(e, search)


@pytest.mark.parametrize("B,n_iso", [(8, 8), (4, 1)])
def test_grey_context_every_lazy_path(counted, lena64, B, n_iso):
    img = np.ascontiguousarray(lena64)
    with fic_amd.Encoder(W, H, B, None, n_iso) as enc:
        created = _alive()
        assert created["pinned_allocations"] == 0
        enc.set_gray(img)
        sweeps = [2] + ([5] if n_iso == 8 else []) + [6] + ([3, 4] if capi.has_xcheck() else [])    # 3 then 4: the operand types
        configs = [(s, 0, 0) for s in sweeps] + [(0, 1, 1), (0, 1, enc.n_domains)]                   # lsq: 1 chunk, then the most
        for sweep, search, chunks in configs:
            _configure(enc, sweep, search, chunks)
            enc.encode()
            _same(_grey_results(enc, search), _fresh_grey(img, B, None, n_iso, sweep, search, chunks), f"sweep {sweep} search {search} chunks {chunks}")
        assert capi.live_memory()["pinned_allocations"] == 1                   # the packed records' host copy, on first read
        _configure(enc, 6, 0, 0)
        want = _fresh_grey(img, B, None, n_iso, 6, 0, 0)
        before = _alive()
        for on in (1, 0, 1):
            enc.set_option("sweep_stats", on)
            assert capi.live_memory()["device_allocations"] == before["device_allocations"] + on
            enc.encode()
            _same(enc.results(), want, f"sweep_stats {on}")
        assert enc.sweep_stats()["waves"] > 0
        enc.set_option("time_sweep", 1)
        enc.encode()
        assert enc.sweep_time()[1] == 1
        enc.set_option("time_sweep", 0)
        col = enc.collage()
        dec1, dec2 = enc.decode(1)[0], enc.decode(2)[0]
        assert col.shape == (1, W * H) and dec1.shape == (1, H, W) and dec2.shape == (1, 2 * H, 2 * W)
        enc.set_gray(img)
        enc.encode()
        _same(enc.results(), want, "set_gray again")
        enc.set_argb(_argb(img))
        enc.encode()
        _same(enc.results(), want, "set_argb")
        assert (enc.collage() == col).all() and (enc.decode(1)[0] == dec1).all()
        assert _alive()["device_bytes"] > created["device_bytes"]
    assert capi.live_memory()["device_allocations"] == 1     # the context is gone; the zoomed decode's arena stays parked
    capi.release_cache()
    assert capi.live_memory() == ZERO
    if n_iso == 1:                       # a windowed search: the generic sweep and its least-squares twin
        with fic_amd.Encoder(W, H, B, 2, 1) as enc:
            enc.set_gray(img)
            for sweep, search in ((1, 0), (1, 1), (0, 0)):
                _configure(enc, sweep, search, 0)
                enc.encode()
                assert enc.info()["sweep_kind"] == 1
                _same(_grey_results(enc, search), _fresh_grey(img, B, 2, 1, sweep, search, 0), f"window, sweep {sweep} search {search}")
            _alive()


# ---- 2. a joint-RGB context -----------------------------------------------------------------------------------------------------
# fic_rgb_ctx_debug_q_host's sizes of RgbEncoder.Q_STORES after a matrix-core encode of a 64 x 64 image, per (B, n_iso), as the
# commit before the owner of device memory reported them (14e0996, recorded once on an MI355X)
RGB_Q_BYTES = {
    (4, 1): (31744, 124, 65536, 1024, 2048, 4), (4, 8): (31744, 124, 98304, 1024, 2048, 4),
    (8, 1): (40960, 40, 131072, 256, 512, 4), (8, 8): (40960, 40, 131072, 256, 512, 4),
}


def _fresh_rgb(argb, B, wK, n_iso, sweep, collage):
    with capi.RgbEncoder(W, H, B, wK, 1, 0, n_iso) as e:
        e.set_option("sweep", sweep)
        e.set_argb(argb)
        e.encode(collage)
        return e.results()


@pytest.mark.parametrize("B,n_iso", [(4, 1), (4, 8), (8, 1), (8, 8)])
def test_rgb_context(counted, B, n_iso):
    argb = _colour()
    wK = capi.geometry(W, H, B)[2]       # full search
    with capi.RgbEncoder(W, H, B, wK, 1, 0, n_iso) as enc:
        _alive()
        enc.set_argb(argb)
        want = {s: _fresh_rgb(argb, B, wK, n_iso, s, False) for s in (1, 2)}
        for sweep in (1, 2, 1):
            enc.set_option("sweep", sweep)
            enc.encode()
            assert enc.last_sweep() == sweep
            _same(enc.results(), want[sweep], f"sweep {sweep}")
            if sweep == 2:
                assert tuple(int(enc.debug_q(w).size) for w in enc.Q_STORES) == RGB_Q_BYTES[(B, n_iso)]
        enc.set_option("sweep", 2)
        before = _alive()
        for on in (1, 0):
            enc.set_option("sweep_stats", on)
            assert capi.live_memory()["device_allocations"] == before["device_allocations"] + on
            enc.encode(True)
            _same(enc.results(), _fresh_rgb(argb, B, wK, n_iso, 2, True), f"collage, sweep_stats {on}")
            if on:
                assert enc.sweep_stats()["waves"] > 0
        dec1, dec2 = enc.decode(1)[0], enc.decode(2)[0]
        assert dec1.shape == (1, W * H) and dec2.shape == (1, 4 * W * H)
        assert _alive()["pinned_allocations"] == 0


# ---- 3. the one-shot entries and their caches -----------------------------------------------------------------------------------
def test_oneshot_caches_evict_and_release(counted):
    """One geometry more than each cache holds (16 grey, 4 joint-RGB): the context that falls out really frees its memory."""
    widths = [32 + 8 * i for i in range(17)]
    counts, last = [], None
    for w in widths:                                     # windowed (wK = 2): every context makes the same allocations
        last = fic_amd.synth.image_u(w, H, 7 + w)
        capi.encode_gray_oneshot(last, 4, 2)
        counts.append(_alive()["device_allocations"])
    per = counts[0]
    assert counts[:16] == [per * (i + 1) for i in range(16)] and counts[16] == counts[15], counts
    assert capi.live_memory()["pinned_allocations"] == 16
    m = capi.live_memory()
    want = capi.encode_gray_oneshot(last, 4, 2)          # the most recent geometry again: its context comes from the cache
    assert capi.live_memory() == m
    _same(capi.encode_gray_oneshot(last, 4, 2), want, "cached grey context")
    capi.release_cache()
    assert capi.live_memory() == ZERO
    counts = []
    for w in widths[:5]:
        argb = _argb(fic_amd.synth.image_u(w, H, 11 + w))
        capi.encode_rgb(argb, w, H, 4, 2)
        counts.append(_alive()["device_allocations"])
    per = counts[0]
    assert counts[:4] == [per * (i + 1) for i in range(4)] and counts[4] == counts[3], counts
    m = capi.live_memory()
    capi.encode_rgb(argb, widths[4], H, 4, 2)
    assert capi.live_memory() == m


# ---- 4. everything else that allocates ------------------------------------------------------------------------------------------
def test_every_other_entry_then_zero(counted, lena64):
    img, argb = np.ascontiguousarray(lena64), _colour()
    streams = []                                         # (decoder, stream)
    leaves = capi.encode_gray_quadtree(img, 16, 4, 0, 8, 200.0)
    streams.append((capi.decode_quadtree_run, capi.write_run_quadtree(leaves, W, H, 16, 4, 0, 8)))
    leaves = capi.encode_rgb_quadtree(argb, W, H, 16, 4, 0, 200.0)
    streams.append((capi.decode_rgb_quadtree_run, capi.write_run_rgb_quadtree(leaves, W, H, 16, 4, 0)))
    leaves = capi.encode_rgb_quadtree_iso(argb, W, H, 16, 4, 0, 8, 200.0)
    streams.append((capi.decode_rgb_quadtree_iso_run, capi.write_run_rgb_quadtree_iso(leaves, W, H, 16, 4, 0)))
    leaves, _, _ = capi.encode_gray_quadtree_budget(img, 16, 4, 0, 1, max_leaves=100)
    assert 16 <= len(leaves) <= 100
    assert len(capi.encode_gray_quadtree(img, 16, 4, 0, 1, 200.0, search="lsq")) >= 16
    _alive()                                             # the levels' contexts are parked in the caches
    g = capi.encode_gray_oneshot(img, 4, 2, 8)
    streams.append((capi.decode_gray_run, capi.write_run_gray(g["qrows"], W, H, 4, 2)))
    streams.append((capi.decode_gray_iso_run, capi.write_run_gray_iso(g["qrows"], g["iso"], W, H, 4, 2)))
    c = capi.encode_rgb(argb, W, H, 4, 2, n_iso=8)
    streams.append((capi.decode_rgb_run, capi.write_run_rgb(c["qrows"], W, H, 4, 2)))
    streams.append((capi.decode_rgb_iso_run, capi.write_run_rgb_iso(c["qrows"], c["iso"], W, H, 4, 2)))
    for fn, run in streams:
        for zoom in (1, 2):
            assert np.asarray(fn(run, zoom=zoom)[0]).size == zoom * zoom * W * H, fn.__name__
    keys = np.arange(1000, dtype=np.uint32) * 7919 % 1000
    assert capi.debug_qt_select(keys, 10)[0] == 989
    roots = np.zeros(100, np.float64)
    capi.check(capi.lib().fic_debug_sqrt_f64(0, 0, 100, roots.ctypes.data_as(C.POINTER(C.c_double))))
    assert roots[81] == 9.0
    vals, out = np.arange(1, 101, dtype=np.uint32), C.c_float()
    capi.check(capi.lib().fic_debug_float_sum(0, C.c_float(0.0), capi.ptr(vals, C.c_uint32), vals.size, C.byref(out)))
    assert out.value == 5050.0
    _same(capi.encode_gray_multi(img, 4, 2, 8, n_gpus=1), g, "multi-device entry on one device")
    _alive()


# ---- 5. a refused call frees its scratch ----------------------------------------------------------------------------------------
def test_refused_calls_free_their_scratch(counted, lena64):
    img = np.ascontiguousarray(lena64)
    L = capi.lib()
    leaves = capi.encode_gray_quadtree(img, 16, 4, 0, 1, 200.0)
    _alive()
    capi.release_cache()                                 # a refused encode destroys its contexts instead of parking them
    before = capi.live_memory()
    assert before == ZERO
    out, n = np.zeros((len(leaves) - 1, 7), np.int32), C.c_int(-1)
    rc = L.fic_encode_gray_quadtree_u8(capi.ptr(img, C.c_uint8), W, H, 16, 4, 0, 1, 200.0, 0, capi.ptr(out, C.c_int32), out.shape[0], C.byref(n))
    assert rc == -8 and n.value == len(leaves) and f"{len(leaves)} leaves, room for {len(leaves) - 1}" in capi.last_error()
    assert capi.live_memory() == before
    # a .run row just outside the window: the paint kernel flags it and the loop refuses the stream
    g = capi.encode_gray_oneshot(img, 4, 2)
    run = capi.write_run_gray(g["qrows"], W, H, 4, 2)
    good = capi.decode_gray_run(run)[0]
    before = _alive()                                    # the arena of this size is parked now
    rows = g["qrows"].copy()
    rows[5, 0] = 2 * 2
    with pytest.raises(fic_amd.FicError) as e:
        capi.decode_gray_run(capi.write_run_gray(rows, W, H, 4, 2))
    assert e.value.code == -3 and "points outside the domain pool" in str(e.value)
    assert capi.live_memory() == before
    assert (capi.decode_gray_run(run)[0] == good).all() and capi.live_memory() == before
