"""Decode and collage of every plane of a batched quadtree handle at once (fic_qt_ctx_decode_zoom_host / _collage_host,
fic_amd.QuadtreeEncoder.decode / .collage).  Plane p of a decode must be, bit for bit, what the one-shot
decoder of the context's format returns for plane p's stream at the same zoom -- image, avgError bits, iterations -- and plane
p of the collage one paint of its leaves from the scaled input: the image whose squared distance from the input is the
encoder's collage SSE, leaf by leaf.  Both work on the tables as they stand on the device, where the caller can write them:
a scribbled table is refused with the plane's number, never read through.  Three unlike planes per batch (constant, noise,
Lena) finish at different iterations; the shapes put several planes inside one would-be workgroup, use a window on a
non-square image, and give two workgroups per plane and float sums above 2^24."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import fic_amd
from fic_amd import capi, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qtmodel as qm  # noqa: E402
import qtrgbmodel as rm  # noqa: E402
import zoommodel as zm  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INF = float("inf")
# w, h, B_max, B_min, wK (0: full search)
SHAPES = [
    (32, 32, 16, 4, 0),       # N_top = 4: several planes inside one would-be workgroup
    (32, 32, 8, 4, 0),        # two levels
    (64, 48, 16, 4, 2),       # not square, a window
    (272, 272, 16, 4, 0),     # two workgroups per plane, two float-sum segments (the second partial), sums above 2^24
]
SHAPE_IDS = [f"{s[0]}x{s[1]}-{s[2]}to{s[3]}-wK{s[4]}" for s in SHAPES]
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
    """The three unlike planes: constant (converges at once), noise (splits everywhere), Lena.  uint8 [3, h, w] or packed ARGB
    int32 [3, h, w]."""
    if not colour:
        lena = np.load(os.path.join(GOLDEN, "lena_grey_256.npy"))
        return np.stack([np.full((h, w), 93, np.uint8), synth.image_u(w, h, 4242 + w).reshape(h, w), _fit(lena, w, h)])
    lena = np.load(os.path.join(GOLDEN, "lena_colored_256.npy"))
    const = np.empty((h, w, 3), np.uint8)
    const[...] = (200, 93, 17)
    noise = np.stack([synth.image_u(w, h, 777 + 31 * c + w).reshape(h, w) for c in range(3)], axis=-1)
    nat = np.stack([_fit(np.ascontiguousarray(lena[..., c]), w, h) for c in range(3)], axis=-1)
    return np.stack([_pack(const), _pack(noise), _pack(nat)])


class _Case:
    def __init__(self, codec, shape):
        self.colour, self.n_iso = codec.startswith("colour"), int(codec[-1])
        self.w, self.h, self.B_max, self.B_min, self.wK = shape
        self.n_top = (self.w // self.B_max) * (self.h // self.B_max)
        self.n_max = (self.w // self.B_min) * (self.h // self.B_min)
        self.imgs = _images(self.colour, self.w, self.h)
        self.iso_col = 8 if self.colour else 6

    def encoder(self, planes=3):
        return fic_amd.QuadtreeEncoder(self.w, self.h, self.B_max, self.B_min, self.wK, self.n_iso, planes, self.colour)

    def set(self, enc, imgs=None):
        (enc.set_argb if self.colour else enc.set_gray)(self.imgs if imgs is None else imgs)

    def oneshot_decode(self, run, zoom):
        return (capi.decode_rgb_quadtree_iso_run if self.colour else capi.decode_quadtree_run)(run, zoom=zoom)

    def mixed_budget(self):
        """RD leaf budgets of about a quarter of Nr_min: trees with leaves of more than one side where the image splits at all."""
        q = max(self.n_max // 4, self.n_top + 3)
        return [q, q + 3, min(self.n_max, q + 9)]


def _bits(x):
    return int(np.float32(x).view(np.uint32))


def _same_as_oneshot(case, enc, what, zooms=(1, 2, 4)):
    """Every plane of enc.decode(zoom) against the one-shot decoder on that plane's stream.  Returns the iterations at zoom 1."""
    runs = enc.write_runs()
    its = None
    for z in zooms:
        if z * case.B_max > 64:
            continue
        img, avg, it = enc.decode(zoom=z)
        assert img.shape == (3, z * case.h, z * case.w) and img.dtype == (np.int32 if case.colour else np.uint8)
        for p in range(3):
            wimg, wavg, wit = case.oneshot_decode(runs[p], z)
            print(f"{what} zoom {z} plane {p}: iterations {it[p]} / {wit}, avgError bits {_bits(avg[p]):#x} / {_bits(wavg):#x}, "
                  f"pixels that differ {int((img[p] != wimg).sum())}")
            assert int(it[p]) == int(wit), f"{what} zoom {z} plane {p}: {it[p]} iterations, the one-shot decoder {wit}"
            assert _bits(avg[p]) == _bits(wavg), f"{what} zoom {z} plane {p}: avgError {avg[p]!r}, the one-shot decoder {wavg!r}"
            assert (img[p] == wimg).all(), f"{what} zoom {z} plane {p}: {int((img[p] != wimg).sum())} pixels differ"
        if z == 1:
            its = [int(x) for x in it]
    return its


@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_decode_is_the_oneshot_decoder_plane_by_plane(shape, codec):
    """A mixed tree (RD leaf budgets of about a quarter of Nr_min), then the two extremes: only B_max leaves (threshold +inf)
    and only B_min leaves (threshold -1); zoom 1, 2 and 4 each."""
    case = _Case(codec, shape)
    with case.encoder() as enc:
        case.set(enc)
        enc.encode(max_leaves=case.mixed_budget())
        sides = {int(b) for leaves, _, _ in enc.results() for b in leaves[:, 2]}
        assert len(sides) >= 2, f"the budget {case.mixed_budget()} gives leaves of the sides {sides} only"
        its = _same_as_oneshot(case, enc, f"{shape} {codec} budget")
        assert len(set(its)) >= 2, f"the planes finish together, after {its} iterations"
        enc.encode(threshold=INF)
        assert [len(r[0]) for r in enc.results()] == [case.n_top] * 3
        _same_as_oneshot(case, enc, f"{shape} {codec} threshold +inf")
        enc.encode(threshold=-1.0)
        assert [len(r[0]) for r in enc.results()][1:] == [case.n_max] * 2
        _same_as_oneshot(case, enc, f"{shape} {codec} threshold -1")


def _fixed_tree(case, plane):
    """int64 [n, 3] leaves {x, y, B} of a mixed tree that depends on nothing but the shape and the plane, in the table's order:
    top blocks in scanline order, children TL, TR, BL, BR depth first.  Top block t splits by the bits of (7 t + 5 plane + 19)
    mod 32: bit 4 the block itself, bit c its child c (three levels only)."""
    rows, t = [], 0
    for y in range(0, case.h, case.B_max):
        for x in range(0, case.w, case.B_max):
            s = (7 * t + 5 * plane + 19) % 32
            t += 1
            if not s & 16:
                rows.append((x, y, case.B_max))
                continue
            hb = case.B_max // 2
            for c, (dx, dy) in enumerate(((0, 0), (hb, 0), (0, hb), (hb, hb))):
                if hb > case.B_min and (s >> c) & 1:
                    q = hb // 2
                    rows += [(x + dx + ex, y + dy + ey, q) for ex, ey in ((0, 0), (q, 0), (0, q), (q, q))]
                else:
                    rows.append((x + dx, y + dy, hb))
    return np.array(rows, np.int64)


def _sqoff(x, y, B, B_max, Rw_top, exchanged):
    """The closed form of DESIGN.md 4.25 for a leaf's place among the squares; exchanged: TR and BL swapped at every level."""
    xr, yr = x % B_max, y % B_max
    px = ((y // B_max) * Rw_top + x // B_max) * B_max * B_max
    s = B_max // 2
    while s >= B:
        hi, lo = (yr & s) != 0, (xr & s) != 0
        if exchanged:
            hi, lo = lo, hi
        px += s * s * (2 * hi + lo)
        s //= 2
    return px


def _avg_error_of(case, tree, sq, exchanged):
    """Java's avgError of one iteration whose squares are sq[i] on every pixel of leaf i: one float32 add per pixel in the
    order of the leaves' places, then the division by the pixel count (FC:407, FC:413)."""
    buf = np.zeros(case.w * case.h, np.float32)
    for (x, y, B), s in zip(tree, sq):
        o = _sqoff(int(x), int(y), int(B), case.B_max, case.w // case.B_max, exchanged)
        buf[o:o + B * B] = s
    acc = np.add.accumulate(np.concatenate([[np.float32(0)], buf]).astype(np.float32), dtype=np.float32)
    return np.float32(acc[-1] / np.float32(case.w * case.h))


@pytest.mark.parametrize("codec", ["grey-iso1", "colour-iso1"])
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3]], ids=[SHAPE_IDS[0], SHAPE_IDS[3]])
def test_the_order_of_the_squares_reaches_avg_error(shape, codec):
    """The squares' place in sqbuf (qt_decode_sqoff in k_qt_resolve) shows in the result only when the float sum of the LAST
    iteration is not exact: a plane that does not converge, with a sum above 2^24.  No encode gives one, so after an encode the
    whole table is written on the device: a fixed mixed tree per plane (_fixed_tree) whose rows carry a map that no encoder
    writes and every decoder takes, a = -3 and a brightness b of 150 .. 249 that differs from leaf to leaf.  From grey 128
    every pixel goes to 0, then to its leaf's b, then (every domain pixel is at least 128) to 0 again, for all 50 iterations,
    with b^2 per pixel and channel.  The float sum of those squares is worked out here in the true order and with TR and BL
    exchanged: the decode must give the first, and the two must differ -- so a decode that placed the squares in the exchanged
    order could not pass."""
    import torch
    case = _Case(codec, shape)
    with case.encoder() as enc:
        case.set(enc)
        enc.encode(threshold=1.0)                                   # any encode: the tables exist, the context may decode
        dev = enc.results_device()
        t = np.zeros(tuple(dev["leaves"].shape), np.int32)
        want, other = [], []
        for p in range(3):
            tree = _fixed_tree(case, p)
            n = len(tree)
            assert len(set(tree[:, 2])) >= 2 and int((tree[:, 2] ** 2).sum()) == case.w * case.h
            b = 150 + (np.arange(n) * 37 + 11 * p) % 100
            t[p, :n, :3] = tree                                     # idx_local 0 and isometry 0: valid at every level
            if case.colour:
                bG, bB = 150 + (b * 7) % 100, 150 + (b * 13) % 100
                t[p, :n, 4] = -3000000                              # a = q1 / 10^6
                t[p, :n, 5] = b * 100000                            # bR = q2 / 10^5
                t[p, :n, 6] = bG * 100000                           # bG = q3 / 10^5
                t[p, :n, 7] = bB                                    # bB = q4
                sq = b * b + bG * bG + bB * bB
            else:
                t[p, :n, 4] = -300                                  # a = qa / 100
                t[p, :n, 5] = b
                sq = b * b
            dev["n_leaves"][p] = n
            want.append(_avg_error_of(case, tree, sq, False))
            other.append(_avg_error_of(case, tree, sq, True))
        differ = [p for p in range(3) if _bits(want[p]) != _bits(other[p])]
        print(f"{shape} {codec}: avgError in the true order {[hex(_bits(x)) for x in want]}, exchanged {[hex(_bits(x)) for x in other]}")
        assert differ, "exchanging TR and BL leaves every plane's float sum as it is: this table cannot tell the orders apart"
        assert all(float(x) * case.w * case.h >= 2 ** 24 for x in want), "a last sum below 2^24 is an exact float: any order gives it"
        dev["leaves"].copy_(torch.from_numpy(t).to(dev["leaves"].device))
        torch.cuda.synchronize()
        its = _same_as_oneshot(case, enc, f"{shape} {codec} oscillating", zooms=(1, 2))
        assert its == [50, 50, 50], f"the planes were to run all 50 iterations, they ran {its}"
        _, avg, _ = enc.decode()
        for p in range(3):
            assert _bits(avg[p]) == _bits(want[p]), f"plane {p}: avgError {avg[p]!r}, the squares summed in the table's order give {want[p]!r}"


def _numpy_collage(case, img, leaves):
    """One paint of the leaves from the scaled original, through the numpy models' paint (tests/zoommodel.py's levels)."""
    hd = dict(w=case.w, h=case.h, B_max=case.B_max, B_min=case.B_min, wK=case.wK)
    lev, w, h = zm._zoomed_levels(hd, leaves, 1)
    if not case.colour:
        out = np.zeros((h, w), np.int64)
        for B, (lv, gi, rr, cc, _) in lev.items():
            out[rr, cc] = qm.paint_values(img, B, gi, lv[:, 4], lv[:, 5], lv[:, 6])
        return out.astype(np.uint8)
    scaled = rm.scale_rgb(rm.channels(img, w, h))
    out = np.zeros((h, w, 3), np.int64)
    for B, (lv, gi, rr, cc, _) in lev.items():
        v = rm.paint_values(scaled, B, gi, lv[:, 3:8])                       # position p from domain position p
        out[rr, cc] = np.take_along_axis(v, qm.iso_table(B)[lv[:, 8]][:, :, None], axis=1)      # ... from iso's source of p
    return rm.pack(out)


def _sq_err(case, a, b):
    """int64 [h, w]: squared distance of two images of the case's format, summed over the channels."""
    if not case.colour:
        d = a.astype(np.int64) - b.astype(np.int64)
        return d * d
    d = rm.channels(a, case.w, case.h) - rm.channels(b, case.w, case.h)
    return (d * d).sum(axis=-1)


@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_collage_is_the_image_behind_the_collage_sse(shape, codec):
    case = _Case(codec, shape)
    with case.encoder() as enc:
        case.set(enc)
        enc.encode(max_leaves=case.mixed_budget())
        res = enc.results()
        col = enc.collage()
    assert col.shape == (3, case.h, case.w) and col.dtype == (np.int32 if case.colour else np.uint8)
    for p in range(3):
        leaves, _, stats = res[p]
        img = case.imgs[p]
        err = _sq_err(case, img, col[p])
        print(f"{shape} {codec} plane {p}: {len(leaves)} leaves, collage SSE {int(err.sum())}, stats {int(stats[0])}")
        assert int(err.sum()) == int(stats[0]), f"plane {p}: the collage is {int(err.sum())} from the input, stats say {int(stats[0])}"
        if case.colour:
            sse = capi.debug_rgb_quadtree_iso_sse(img.reshape(-1), case.w, case.h, case.B_max, case.B_min, case.wK, case.n_iso)
        else:
            sse = capi.debug_quadtree_sse(img, case.B_max, case.B_min, case.wK, case.n_iso)
        for x, y, B in leaves[:, :3]:
            got = int(err[y:y + B, x:x + B].sum())
            assert got == int(sse[B][y // B, x // B]), f"plane {p} leaf ({x}, {y}, {B}): SSE {got}, the level's {int(sse[B][y // B, x // B])}"
        want = _numpy_collage(case, img, leaves)
        assert (col[p] == want).all(), f"plane {p}: {int((col[p] != want).sum())} pixels differ from the numpy paint"


@pytest.mark.parametrize("codec", ["grey-iso8", "colour-iso1"])
def test_planes_are_independent_and_a_second_encode_shows(codec):
    """Permuting the input planes permutes the outputs; after a second encode with another rule decode() shows the new tables."""
    case = _Case(codec, SHAPES[3])
    M = [400, 2000, 1000]
    perm = [2, 0, 1]
    with case.encoder() as enc:
        case.set(enc)
        enc.encode(max_leaves=M)
        a, a_col = enc.decode(), enc.collage()
        case.set(enc, case.imgs[perm])
        enc.encode(max_leaves=[M[p] for p in perm])
        b, b_col = enc.decode(), enc.collage()
        for i, p in enumerate(perm):
            assert (b[0][i] == a[0][p]).all() and _bits(b[1][i]) == _bits(a[1][p]) and b[2][i] == a[2][p], f"plane {i} of the permuted batch"
            assert (b_col[i] == a_col[p]).all(), f"collage of plane {i} of the permuted batch"
        assert len({int(x) for x in a[2]}) >= 2, "the planes are unlike each other"
        enc.encode(lam=[0, 5000, 100000])
        c = enc.decode()
        assert any((c[0][i] != b[0][i]).any() for i in range(3)), "the second encode changed nothing"
        _same_as_oneshot(case, enc, f"{codec} after a second encode", zooms=(1,))


SCRIBBLES = ("idx_local", "side", "x", "iso", "duplicate", "n_leaves", "hole")


@pytest.mark.parametrize("codec", ["grey-iso1", "grey-iso8", "colour-iso1", "colour-iso8"])
def test_scribbled_tables_are_refused_by_plane_and_never_read_through(codec):
    """The tables lie where the caller can write them (results_device()).  Each scribble on plane 1: decode() and collage()
    raise FIC_E_ARGUMENT naming the plane, and the context then encodes and decodes correctly again."""
    import torch
    case = _Case(codec, SHAPES[2])                                  # wK = 2 at every level: idx_local 4 is the first one outside
    with case.encoder() as enc:
        case.set(enc)
        enc.encode(max_leaves=case.mixed_budget())
        good = enc.decode()
        good_col = enc.collage()
        dev = enc.results_device()
        for what in SCRIBBLES:
            leaves, n = dev["leaves"], dev["n_leaves"]
            row = 5
            if what == "idx_local":
                leaves[1, row, 3] = case.wK * case.wK
            elif what == "side":
                leaves[1, row, 2] = 5
            elif what == "x":
                leaves[1, row, 0] = case.w
            elif what == "iso":
                leaves[1, row, case.iso_col] = case.n_iso
            elif what == "duplicate":
                leaves[1, row + 1] = leaves[1, row].clone()
            elif what == "n_leaves":
                n[1] = 0
            else:
                n[1] = n[1] - 1                                     # the last leaf's cells stay uncovered
            torch.cuda.synchronize()
            for zoom in (1, 2):
                with pytest.raises(fic_amd.FicError) as e:
                    enc.decode(zoom=zoom)
                assert e.value.code == -3 and "plane 1" in str(e.value), f"{what}, zoom {zoom}: {e.value}"
            with pytest.raises(fic_amd.FicError) as e:
                enc.collage()
            assert e.value.code == -3 and "plane 1" in str(e.value), f"{what}: {e.value}"
            enc.encode(max_leaves=case.mixed_budget())
            again = enc.decode()
            assert (again[0] == good[0]).all() and (again[1].view(np.uint32) == good[1].view(np.uint32)).all() and (again[2] == good[2]).all(), what
            assert (enc.collage() == good_col).all(), what
        _same_as_oneshot(case, enc, f"{codec} after the scribbles", zooms=(1, 2))


def test_refusals():
    case = _Case("grey-iso1", SHAPES[0])
    L = capi.lib()
    with case.encoder() as enc:
        case.set(enc)
        for call in (enc.decode, enc.collage):                      # before the first encode
            with pytest.raises(fic_amd.FicError) as e:
                call()
            assert e.value.code == -7, str(e.value)
        enc.encode(lam=[5, 50, 500])
        good = enc.decode()
        for zoom in (0, 3, 8, -1):
            with pytest.raises(fic_amd.FicError) as e:
                enc.decode(zoom=zoom)
            assert e.value.code == -3, (zoom, str(e.value))
        out = np.zeros((3, 32, 32), np.uint8)
        avg, it = np.zeros(3, np.float32), np.zeros(3, np.int32)
        args = (capi.ptr(avg, C.c_float), capi.ptr(it, C.c_int))
        for zoom in (0, 3, 8):                                      # the library's own refusal, whatever room it is promised
            assert L.fic_qt_ctx_decode_zoom_host(enc._h, zoom, out.ctypes.data_as(C.c_void_p), 1 << 40, *args) == -3, zoom
        assert L.fic_qt_ctx_decode_zoom_host(enc._h, 1, out.ctypes.data_as(C.c_void_p), out.size - 1, *args) == -8
        assert L.fic_qt_ctx_decode_zoom_host(enc._h, 2, out.ctypes.data_as(C.c_void_p), 4 * out.size - 1, *args) == -8
        assert L.fic_qt_ctx_collage_host(enc._h, out.ctypes.data_as(C.c_void_p), out.size - 1) == -8
        assert L.fic_qt_ctx_decode_zoom_host(enc._h, 1, None, out.size, *args) == -3
        assert L.fic_qt_ctx_collage_host(enc._h, None, out.size) == -3
        assert L.fic_qt_ctx_decode_zoom_host(None, 1, out.ctypes.data_as(C.c_void_p), out.size, *args) == -3
        assert not out.any() and not avg.any() and not it.any(), "a refused call wrote"
        # avg_error_out and iterations_out may be NULL; the refusals left the context as it was
        assert L.fic_qt_ctx_decode_zoom_host(enc._h, 1, out.ctypes.data_as(C.c_void_p), out.size, None, None) == 0
        assert (out == good[0]).all()


def test_no_memory_is_left_behind():
    case = _Case("colour-iso8", SHAPES[0])
    enc = case.encoder()
    case.set(enc)
    enc.encode(max_sse=[10, 0, 10 ** 7])
    enc.decode()
    enc.decode(zoom=2)                                              # an arena of the decode jobs
    enc.collage()
    live = capi.live_memory()
    assert live["device_bytes"] > 0
    enc.close()
    capi.release_cache()
    live = capi.live_memory()
    assert all(v == 0 for v in live.values()), live
