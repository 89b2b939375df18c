"""The batched quadtree encoder handle (fic_qt_ctx_*, fic_amd.QuadtreeEncoder) against the one-shot entries:
plane p of a batch must be, bit for bit, what the one-shot entry of the same format returns for image p alone -- the leaf count,
the rows, the threshold's bits or lambda, the statistics -- for every split rule, both searches, grey and colour with 1 and 8
isometries, on shapes at which a kernel that let a workgroup run from one plane into the next would show.  Then the planes'
independence, the device-pointer contract, the refusals, the streams and the lifetime of the memory."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import fic_amd
from fic_amd import capi, synth

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INF = float("inf")
LAM_MAX = (1 << 32) - 1
# w, h, B_max, B_min, wK (0: full search, which needs square block grids)
SHAPES = [
    (32, 32, 16, 4, 0),       # N_top = 4: three planes inside what a flattened launch would make one workgroup
    (32, 32, 8, 4, 0),        # N_top = 16, two levels
    (64, 48, 16, 4, 2),       # N_top = 12, not square, a window
    (272, 272, 16, 4, 0),     # N_top = 289: two workgroups per plane, the second partial; 289 + 1156 keys, 4624 leaves at most
    (256, 256, 16, 8, 0),     # the golden images as they are: two levels, no keys of level 1
]
CODECS = ("grey-iso1", "grey-iso8", "colour-iso1", "colour-iso8")


def _pack(rgb):
    r, g, b = (rgb[..., i].astype(np.uint32) for i in range(3))
    return np.ascontiguousarray((np.uint32(0xFF000000) | (r << 16) | (g << 8) | b).view(np.int32))


def _fit(base, w, h, oy=0, ox=0):
    """A Lena crop (it fits) or enlargement (it does not)."""
    H, W = base.shape
    if h > H or w > W:
        return synth.enlarge(base, w, h, oy, ox)
    y, x = min(96, H - h), min(64, W - w)
    return np.ascontiguousarray(base[y:y + h, x:x + w])


@functools.lru_cache(maxsize=None)
def _images(colour, w, h):
    """The three unlike planes: constant (no split, every key 0), noise (splits everywhere), Lena.  uint8 [3, h, w] or packed
    ARGB int32 [3, h, w]."""
    if not colour:
        lena = np.load(os.path.join(GOLDEN, "lena_grey_256.npy"))
        return np.stack([np.full((h, w), 93, np.uint8), synth.image_u(w, h, 4242 + w).reshape(h, w), _fit(lena, w, h)])
    lena = np.load(os.path.join(GOLDEN, "lena_colored_256.npy"))
    const = np.empty((h, w, 3), np.uint8)
    const[...] = (200, 93, 17)
    noise = np.stack([synth.image_u(w, h, 777 + 31 * c + w).reshape(h, w) for c in range(3)], axis=-1)
    nat = np.stack([_fit(np.ascontiguousarray(lena[..., c]), w, h) for c in range(3)], axis=-1)
    return np.stack([_pack(const), _pack(noise), _pack(nat)])


class _OneShot:
    """The reference of every comparison: the one-shot entries of one format on one image."""

    def __init__(self, codec, shape, search):
        self.colour, self.n_iso = codec.startswith("colour"), int(codec[-1])
        self.w, self.h, self.B_max, self.B_min, self.wK = shape
        self.search = search
        self.cols = 9 if self.colour else 7

    def _head(self, img):
        if self.colour:
            return (img.reshape(-1), self.w, self.h, self.B_max, self.B_min, self.wK, self.n_iso)
        return (img, self.B_max, self.B_min, self.wK, self.n_iso)

    def threshold(self, img, t):
        fn = capi.encode_rgb_quadtree_iso if self.colour else capi.encode_gray_quadtree
        return fn(*self._head(img), threshold=t, search=self.search)

    def budget(self, img, M):
        fn = capi.encode_rgb_quadtree_iso_budget if self.colour else capi.encode_gray_quadtree_budget
        return fn(*self._head(img), max_leaves=M)

    def rd(self, img, **goal):
        fn = capi.encode_rgb_quadtree_iso_rd if self.colour else capi.encode_gray_quadtree_rd
        return fn(*self._head(img), search=self.search, **goal)

    def write(self, leaves):
        if self.colour:
            return capi.write_run_rgb_quadtree_iso(leaves, self.w, self.h, self.B_max, self.B_min, self.wK)
        return capi.write_run_quadtree(leaves, self.w, self.h, self.B_max, self.B_min, self.wK, self.n_iso)

    def decode(self, run):
        return (capi.decode_rgb_quadtree_iso_run if self.colour else capi.decode_quadtree_run)(run)


def _encoder(ref, planes):
    return fic_amd.QuadtreeEncoder(ref.w, ref.h, ref.B_max, ref.B_min, ref.wK, ref.n_iso, planes, ref.colour)


def _set(enc, imgs):
    (enc.set_argb if enc.colour else enc.set_gray)(imgs)


def _bits(x):
    return int(np.float32(x).view(np.uint32))


def _same(got, want, what, threshold_rule):
    """One plane of a batch against the one-shot's (leaves, param, stats); stats None: the one-shot entry has none."""
    leaves, param, stats = got
    wl, wp, ws = want
    assert len(leaves) == len(wl), f"{what}: {len(leaves)} leaves, the one-shot entry {len(wl)}"
    assert leaves.shape == wl.shape and (leaves == wl).all(), f"{what}: rows differ, first at {np.nonzero((leaves != wl).any(axis=1))[0][:5]}"
    if threshold_rule:
        assert _bits(param) == _bits(wp), f"{what}: threshold {param!r}, the one-shot entry {wp!r}"
    else:
        assert int(param) == int(wp), f"{what}: lambda {param}, the one-shot entry {wp}"
    if ws is not None:
        assert (stats == ws).all(), f"{what}: stats {stats.tolist()}, the one-shot entry {ws.tolist()}"


def _level_counts(leaves, B_max):
    return [int((leaves[:, 2] == B_max >> l).sum()) for l in range(3)]


@pytest.mark.parametrize("search", ["reference", "lsq"])
@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{s[0]}x{s[1]}-{s[2]}to{s[3]}-wK{s[4]}" for s in SHAPES])
def test_every_rule_matches_the_oneshot_entries(shape, codec, search):
    """planes 1 and 3, the five rules, per-plane values that differ between the planes."""
    ref = _OneShot(codec, shape, search)
    w, h, B_max, B_min, _ = shape
    n_top, n_max = (w // B_max) * (h // B_max), (w // B_min) * (h // B_min)
    imgs = _images(ref.colour, w, h)
    d0 = int(ref.rd(imgs[2], lam=0)[2][0])                      # Lena's smallest collage SSE on this ladder
    values = {                                                  # per plane: constant, noise, Lena
        "threshold": [INF, -1.0, 40.0],
        "budget": [n_top, n_max, (n_top + n_max) // 2],
        "lam": [0, LAM_MAX, 300],
        "max_leaves": [n_max, n_top, (n_top + n_max) // 2],
        "max_sse": [10, 0, 2 * d0 + 1000],                      # out of reach on the noise plane
    }
    rules = [r for r in values if not (r == "budget" and search == "lsq")]

    @functools.lru_cache(maxsize=None)
    def want(rule, p):
        v = values[rule][p]
        if rule == "threshold":
            leaves = ref.threshold(imgs[p], v)
            return leaves, np.float32(v), None
        if rule == "budget":
            return ref.budget(imgs[p], v)
        return ref.rd(imgs[p], **{rule: v})

    for planes, which in ((3, [0, 1, 2]), (1, [2]), (1, [1])):
        with _encoder(ref, planes) as enc:
            enc.set_option("search", search)
            _set(enc, imgs[which])
            for rule in rules:
                v = [values[rule][p] for p in which]
                if rule == "budget":
                    enc.encode(max_leaves=v, prune="threshold")
                else:
                    enc.encode(**{rule: v if planes > 1 else v[0]})      # a scalar serves all planes
                got = enc.results()
                assert len(got) == planes
                for i, p in enumerate(which):
                    what = f"{shape} {codec} {search} {rule} = {values[rule][p]} planes {planes} plane {i}"
                    _same(got[i], want(rule, p), what, rule in ("threshold", "budget"))
                    leaves, param, stats = got[i]
                    # the statistics also where the one-shot entry returns none: the leaves per level, the tree at +inf
                    assert stats[1:].tolist() == _level_counts(leaves, B_max) and n_top <= len(leaves) <= n_max, what
                    if rule == "threshold" and values[rule][p] == INF:
                        assert len(leaves) == n_top and (stats == ref.rd(imgs[p], lam=LAM_MAX)[2]).all(), what
                    if rule == "threshold" and values[rule][p] == -1.0:
                        assert len(leaves) == n_max, what
                    if rule == "max_sse" and p == 1:
                        assert param == 0 and int(stats[0]) > values[rule][p], f"{what}: the target is out of reach"
                    if rule == "max_sse" and p == 2:
                        assert int(stats[0]) <= values[rule][p], what


def _grey_case():
    ref = _OneShot("grey-iso1", SHAPES[0], "reference")
    return ref, _images(False, 32, 32)


@pytest.mark.parametrize("codec", ["grey-iso8", "colour-iso1"])
def test_permuting_the_planes_permutes_the_results(codec):
    shape = SHAPES[3]
    ref = _OneShot(codec, shape, "reference")
    imgs = _images(ref.colour, shape[0], shape[1])
    M = [400, 2000, 1000]
    with _encoder(ref, 3) as enc:
        _set(enc, imgs)
        enc.encode(max_leaves=M)
        a = enc.results()
        perm = [2, 0, 1]
        _set(enc, imgs[perm])
        enc.encode(max_leaves=[M[p] for p in perm])
        b = enc.results()
    for i, p in enumerate(perm):
        _same(b[i], a[p], f"{codec}: plane {i} of the permuted batch", False)
    assert len({len(x[0]) for x in a}) >= 2, "the planes are unlike each other"


def test_device_tensor_is_read_in_place_at_encode_time_and_planes_are_isolated():
    """A torch tensor is used where it is: what is written to it after set_gray and before the encode is what gets encoded; a
    change to one plane's pixels changes that plane's outputs only."""
    import torch
    shape = SHAPES[3]
    ref = _OneShot("grey-iso1", shape, "reference")
    imgs = _images(False, 272, 272)
    with _encoder(ref, 3) as enc:
        t = torch.zeros((3, 272, 272), dtype=torch.uint8, device="cuda")
        enc.set_gray(t)
        assert enc._keep is t
        t.copy_(torch.from_numpy(imgs))                              # after set_gray
        torch.cuda.synchronize()
        enc.encode(lam=[200, 200, 200])
        first = enc.results()
        for p in range(3):
            _same(first[p], ref.rd(imgs[p], lam=200), f"plane {p} written after set_gray", False)
        other = synth.image_s(272, 272, 99).reshape(272, 272)
        t[1].copy_(torch.from_numpy(other))
        torch.cuda.synchronize()
        enc.encode(lam=[200, 200, 200])
        second = enc.results()
        _same(second[0], first[0], "plane 0 after plane 1 changed", False)
        _same(second[2], first[2], "plane 2 after plane 1 changed", False)
        _same(second[1], ref.rd(other, lam=200), "plane 1 after it changed", False)
        assert second[1][0].shape != first[1][0].shape or (second[1][0] != first[1][0]).any()


def test_misaligned_view_is_refused_by_the_library_and_cloned_by_the_wrapper():
    import torch
    ref, imgs = _grey_case()
    n = imgs.size
    with _encoder(ref, 3) as enc:
        buf = torch.zeros(n + 8, dtype=torch.uint8, device="cuda")
        view = buf[3:3 + n].view(3, 32, 32)
        view.copy_(torch.from_numpy(imgs))
        torch.cuda.synchronize()
        assert view.data_ptr() % 8 != 0
        assert capi.lib().fic_qt_ctx_set_gray_device(enc._h, C.c_void_p(view.data_ptr())) == -3 and "alignment" in capi.last_error()
        with pytest.raises(fic_amd.FicError) as e:              # nothing is in force yet: the refusal left it so
            enc.encode(threshold=1.0)
        assert e.value.code == -7
        enc.set_gray(view)
        assert enc._keep is not view and enc._keep.data_ptr() % 8 == 0
        enc.encode(threshold=[INF, -1.0, 25.0])
        got = enc.results()
        for p, t in enumerate([INF, -1.0, 25.0]):
            _same(got[p], (ref.threshold(imgs[p], t), np.float32(t), None), f"cloned view, plane {p}", True)
    cref = _OneShot("colour-iso1", SHAPES[0], "reference")
    with _encoder(cref, 1) as enc:
        t = torch.zeros(32 * 32 + 1, dtype=torch.int32, device="cuda")
        assert capi.lib().fic_qt_ctx_set_argb_device(enc._h, C.c_void_p(t.data_ptr() + 2)) == -3 and "alignment" in capi.last_error()
        assert capi.lib().fic_qt_ctx_set_gray_device(enc._h, C.c_void_p(t.data_ptr())) == -3        # a colour context takes ARGB
        cimg = _images(True, 32, 32)[2]
        t[:1024].copy_(torch.from_numpy(cimg.reshape(-1)))
        torch.cuda.synchronize()
        enc.set_argb(t[:1024])
        enc.encode(lam=50)
        _same(enc.results()[0], cref.rd(cimg, lam=50), "colour device tensor", False)


def test_two_streams_last_call_wins_and_result_pointers_never_move():
    import torch
    ref, imgs = _grey_case()
    with _encoder(ref, 3) as enc:
        ptrs = lambda: {k: v.data_ptr() for k, v in enc.results_device().items()}      # noqa: E731
        before = ptrs()
        enc.set_gray(torch.from_numpy(imgs).cuda())
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        enc.encode(threshold=-1.0, stream=s1)
        enc.encode(lam=[0, 100, 1000], stream=s2)
        enc.sync()
        got = enc.results()
        for p, lam in enumerate([0, 100, 1000]):
            _same(got[p], ref.rd(imgs[p], lam=lam), f"plane {p}: the encode on the second stream", False)
        dev = enc.results_device()
        n = dev["n_leaves"].cpu().numpy()
        assert n.tolist() == [len(x[0]) for x in got] and dev["param"].cpu().numpy().tolist() == [0, 100, 1000]
        for p in range(3):
            assert (dev["leaves"][p, :n[p]].cpu().numpy() == got[p][0]).all() and (dev["stats"][p].cpu().numpy().astype(np.uint64) == got[p][2]).all()
        assert ptrs() == before
        for kw in ({"threshold": 3.0}, {"max_leaves": 40, "prune": "threshold"}, {"lam": 7}, {"max_leaves": 40}, {"max_sse": 10 ** 6}):
            enc.encode(**kw, stream=s1)
            enc.sync()
            assert ptrs() == before, kw
        del s1, s2                                                  # after sync nothing waits for them again
        enc.encode(threshold=3.0)
        assert len(enc.results()) == 3


def test_refusals_come_before_any_device_work_and_leave_the_context_usable():
    ref, imgs = _grey_case()
    for bad in ((4, 4), (16, 16), (8, 16), (32, 4)):
        with pytest.raises(fic_amd.FicError) as e:
            fic_amd.QuadtreeEncoder(32, 32, bad[0], bad[1])
        assert e.value.code == -3, bad
    with pytest.raises(fic_amd.FicError) as e:
        fic_amd.QuadtreeEncoder(40, 32, 16, 4)
    assert e.value.code == -1
    with pytest.raises(fic_amd.FicError) as e:                  # 65535 planes of 4624 rows of 9 ints pass 2^31 - 1
        fic_amd.QuadtreeEncoder(272, 272, 16, 4, planes=65535, colour=True)
    assert e.value.code == -1 and "2^31" in str(e.value)
    with pytest.raises(fic_amd.FicError) as e:
        fic_amd.QuadtreeEncoder(32, 32, 16, 4, planes=65536)
    assert e.value.code == -1
    with _encoder(ref, 3) as enc:
        def refused(code, **kw):
            with pytest.raises(fic_amd.FicError) as e:
                enc.encode(**kw)
            assert e.value.code == code, (kw, str(e.value))
        refused(-7, threshold=1.0)                              # no input yet
        enc.set_gray(imgs)
        enc.encode(lam=[5, 50, 500])
        good = enc.results()
        refused(-3, threshold=[1.0, float("nan"), 2.0])
        refused(-3, max_leaves=[4, 3, 64], prune="threshold")   # below N_top = 4 on one plane
        refused(-3, max_leaves=[64, 4, 3])
        refused(-3, lam=[0, LAM_MAX + 1, 0])
        assert capi.lib().fic_qt_ctx_encode_rd(enc._h, 3, capi.ptr(np.zeros(3, np.uint64), C.c_uint64), None) == -3
        enc.set_option("search", "lsq")
        refused(-3, max_leaves=[64, 64, 64], prune="threshold") # the threshold budget has the reference criterion only
        enc.set_option("search", "reference")
        with pytest.raises(fic_amd.FicError):
            enc.set_option("search", 2)
        with pytest.raises(fic_amd.FicError):
            enc.set_option("sweep", 1)
        # none of them touched the results of the last good encode
        for p in range(3):
            _same(enc.results()[p], good[p], f"plane {p} after the refusals", False)
        # a leaf buffer that is too small: FIC_E_CAPACITY, the count is set, nothing is written
        n_want = len(good[2][0])
        out = np.zeros((n_want, 7), np.int32)
        n = C.c_int(-1)
        assert capi.lib().fic_qt_ctx_get_leaves_host(enc._h, 2, capi.ptr(out, C.c_int32), n_want - 1, C.byref(n)) == -8
        assert n.value == n_want and not out.any()
        assert capi.lib().fic_qt_ctx_get_leaves_host(enc._h, 3, capi.ptr(out, C.c_int32), n_want, C.byref(n)) == -3
        assert capi.lib().fic_qt_ctx_get_leaves_host(enc._h, 2, capi.ptr(out, C.c_int32), n_want, C.byref(n)) == 0 and (out == good[2][0]).all()
        enc.encode(max_leaves=[4, 64, 31], prune="threshold")
        got = enc.results()
        for p, M in enumerate([4, 64, 31]):
            _same(got[p], ref.budget(imgs[p], M), f"plane {p}: a budget after the refusals", True)


@pytest.mark.parametrize("codec", ["grey-iso8", "colour-iso8"])
def test_streams_are_the_oneshot_streams_byte_for_byte(codec):
    shape = SHAPES[2]
    ref = _OneShot(codec, shape, "reference")
    imgs = _images(ref.colour, shape[0], shape[1])
    M = [12, 192, 90]
    with _encoder(ref, 3) as enc:
        _set(enc, imgs)
        enc.encode(max_leaves=M)
        runs = enc.write_runs()
        by_bytes = [len(r) for r in runs]
        enc.encode(max_bytes=by_bytes)                          # the same budgets, given as stream sizes
        assert enc.write_runs() == runs
    for p in range(3):
        want = ref.write(ref.rd(imgs[p], max_leaves=M[p])[0])
        assert runs[p] == want, f"{codec}: the stream of plane {p}"
    got, avg, it = ref.decode(runs[2])
    wgot, wavg, wit = ref.decode(ref.write(ref.rd(imgs[2], max_leaves=M[2])[0]))
    assert (got == wgot).all() and _bits(avg) == _bits(wavg) and it == wit and got.shape[:2] == (shape[1], shape[0])


def test_argb_host_input_of_a_grey_context():
    ref, imgs = _grey_case()
    argb = np.stack([fic_amd.RasterImage.from_gray(g).argb.reshape(32, 32) for g in imgs])
    with _encoder(ref, 3) as enc:
        enc.set_argb(argb)
        enc.encode(lam=[10, 20, 30])
        got = enc.results()
    for p, lam in enumerate([10, 20, 30]):
        _same(got[p], ref.rd(imgs[p], lam=lam), f"plane {p} from ARGB", False)


def test_no_memory_is_left_behind():
    ref = _OneShot("colour-iso8", SHAPES[0], "lsq")
    imgs = _images(True, 32, 32)
    enc = _encoder(ref, 3)
    enc.set_option("search", "lsq")
    enc.set_argb(imgs)
    enc.encode(max_sse=[10, 0, 10 ** 7])
    assert len(enc.results()) == 3
    live = capi.live_memory()
    assert live["device_bytes"] > 0 and live["pinned_bytes"] > 0
    enc.close()
    capi.release_cache()
    live = capi.live_memory()
    assert all(v == 0 for v in live.values()), live
