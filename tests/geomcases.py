"""Deterministic geometry cases for the colour and quadtree encoders: the fixed tables of minimum and quadtree geometries, a
seeded fuzz list (FIC_FUZZ_SEED, default 20261004; FIC_FUZZ_CASES, default 40), the images of every case and the CPU
references of every case, computed once per process and shared by test_geometry_cases_model.py (CPU) and the two GPU files
test_gpu_rgb_geometry.py / test_gpu_quadtree_geometry.py.  Every list is built at import time, so every case is its own pytest
id, and the id spells out w, h, B, wK, n_iso, kind, seed and planes: a failing case is reproduced from its name.  The generator
only produces geometries the library accepts (test_geometry_cases_model.py checks it): no test skips or filters a case.
Not a test module; test infrastructure only."""
import os
from collections import namedtuple
from functools import lru_cache

import numpy as np

import fic_amd  # noqa: F401  (the import shim of the package)
import isostreammodel as im
import qtmodel as qm
import qtrgbmodel as qr
import rgbisomodel as rim
from fic_amd import synth
from oracle import fic_oracle as fo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KINDS = ("U", "S", "noise", "low", "ramp", "const", "lena")

Case = namedtuple("Case", "w h B wK n_iso kind seed planes")
QtCase = namedtuple("QtCase", "w h B_max B_min wK kind seed")


def case_id(c):
    return f"w{c.w}-h{c.h}-B{c.B}-wK{c.wK}-iso{c.n_iso}-{c.kind}-s{c.seed}-p{c.planes}"


def qt_case_id(c):
    return f"w{c.w}-h{c.h}-B{c.B_max}_{c.B_min}-wK{c.wK}-{c.kind}-s{c.seed}"


def dims(c):
    """(Rw, Rh, Dw, Dh) of a fixed-B case, as the reference derives them (FC:111-116, FC:1019-1022)."""
    Rw, Rh = c.w // c.B, c.h // c.B
    return Rw, Rh, 2 * Rw - 3, 2 * Rh - 3


def is_full(c):
    """Full search as the library sees it: the window is the whole pool (also a 1 x 1 pool with wK = 1)."""
    Rw, Rh, Dw, Dh = dims(c)
    return c.wK == Dw == Dh


# ---- the fixed tables ---------------------------------------------------------------------------------------------------------
MIN_GEOMETRIES = [  # w, h, B, wK: Rw or Rh = 2 (Dw or Dh = 1), one and two column tiles of the matrix-core mode, W != H both ways
    (8, 8, 4, 1), (16, 16, 8, 1), (32, 32, 16, 1), (12, 12, 4, 1), (12, 12, 4, 3), (24, 24, 8, 2), (24, 24, 8, 3),
    (48, 48, 16, 3), (32, 16, 8, 1), (16, 32, 8, 1), (48, 16, 8, 1), (20, 8, 4, 1), (64, 32, 16, 1), (32, 64, 16, 1),
]
QT_GEOMETRIES = [  # w, h, B_max, B_min, wK
    (16, 16, 8, 4, 1), (32, 32, 16, 4, 1), (32, 32, 16, 8, 0), (48, 32, 16, 4, 1), (32, 64, 16, 8, 1), (96, 64, 16, 4, 3),
    (64, 96, 8, 4, 5), (80, 80, 16, 4, 0), (112, 80, 16, 4, 2),
]
QT_ENCODERS = ("grey-iso1", "grey-iso8", "rgb", "rgbiso-iso1", "rgbiso-iso8")     # tag 2, tag 2, tag 3, tag 6, tag 6

# full-range noise, two planes: the batch path at the smallest sizes too
MIN_CASES = [Case(w, h, B, wK, n_iso, "noise", 7000 + 13 * w + h + wK, 2) for (w, h, B, wK) in MIN_GEOMETRIES for n_iso in (1, 8)]
QT_CASES = [QtCase(w, h, B_max, B_min, wK, kind, 9000 + 5 * w + h + wK) for (w, h, B_max, B_min, wK) in QT_GEOMETRIES
            for kind in ("noise", "S")]


# ---- the seeded fuzz list -----------------------------------------------------------------------------------------------------
def _fuzz(seed, count):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        B = int(rng.choice([4, 8, 16]))
        lim = min(24, 160 // B)
        Rw, Rh = int(rng.integers(2, lim + 1)), int(rng.integers(2, lim + 1))
        if rng.random() < 0.5:
            Rh = Rw
        want_full = Rw == Rh and rng.random() < 0.5
        n_iso = int(rng.choice([1, 8]))
        wK = 2 * Rw - 3 if want_full else int(rng.integers(1, min(2 * Rw - 3, 2 * Rh - 3, 17) + 1))
        if n_iso == 8 and Rw == Rh and wK == 2 * Rw - 3 and Rw * B > 96:     # bounds the numpy model's time (the whole pool x 8)
            Rw = Rh = int(rng.integers(2, 96 // B + 1))
            wK = 2 * Rw - 3
        planes = int(rng.choice([1, 2, 3]))
        kind = str(rng.choice(KINDS))
        out.append(Case(Rw * B, Rh * B, B, wK, n_iso, kind, int(rng.integers(1, 1 << 30)), planes))
    return out


# Appended to every fuzz list: what the coverage conditions of test_geometry_cases_model.py ask for must not hang on the seed.
FUZZ_FIXED = [
    Case(64, 64, 16, 5, 8, "const", 11, 2),       # B = 16 full search with 8 isometries, every error a tie
    Case(40, 40, 4, 17, 8, "low", 12, 1),         # low-depth ties through k_sweep_rgb_fast_iso<16>
    Case(56, 56, 8, 11, 1, "S", 13, 3),           # full search with one isometry, flat blocks
    Case(24, 8, 4, 1, 8, "lena", 14, 2),          # Rh = 2, W > H
    Case(16, 72, 8, 1, 1, "ramp", 15, 1),         # Rw = 2, H > W
    Case(144, 80, 16, 4, 8, "U", 16, 3),          # windowed, W > H, three planes
    Case(48, 32, 8, 2, 8, "const", 17, 2),        # every pair of the window ties in k_sweep_rgb_iso: (c, k) = (0, 0) must win
]

FUZZ_SEED = int(os.environ.get("FIC_FUZZ_SEED", "20261004"))
FUZZ_CASES = _fuzz(FUZZ_SEED, int(os.environ.get("FIC_FUZZ_CASES", "40"))) + FUZZ_FIXED
RGB_CASES = MIN_CASES + FUZZ_CASES


# ---- images -------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _lena():
    return np.load(os.path.join(GOLDEN, "lena_colored_256.npy"))


def rgb_image(kind, w, h, seed, plane):
    """uint8 [h, w, 3] of image `plane` of a case: another image for every plane (plane = `planes` is the extra image of the
    stale-state pass)."""
    s = seed + 7919 * plane
    rng = np.random.default_rng(s)
    if kind in ("U", "S"):          # S: flat blocks, exact ties, 0 / 0 fits
        return np.stack([synth.image(kind, w, h, s + 101 * c) for c in range(3)], axis=-1)
    if kind == "noise":             # full range: kovarianz leaves 2^24 at B = 8 / 16, the accumulation order shows
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "low":               # 1-2-bit channels in 1 / 2 / 4-pixel cells: exact error ties, the strict '<' keeps the lower (c, k)
        bits, cell = 1 + s % 2, (1, 2, 4)[(s // 2) % 3]
        low = rng.integers(0, 1 << bits, (-(-h // cell), -(-w // cell), 3), dtype=np.uint8)
        return (np.repeat(np.repeat(low, cell, 0), cell, 1)[:h, :w] * (255 // ((1 << bits) - 1))).astype(np.uint8)
    if kind == "ramp":
        y, x = np.mgrid[0:h, 0:w]
        return np.stack([(x * 3 + s) % 256, (y * 5 + x + s) % 256, (x + y + 2 * s) % 256], -1).astype(np.uint8)
    if kind == "const":
        return np.full((h, w, 3), (s % 256, (s >> 8) % 256, (s >> 16) % 256), np.uint8)
    if kind == "lena":
        x0, y0 = int(rng.integers(0, 256 - w + 1)), int(rng.integers(0, 256 - h + 1))
        return np.ascontiguousarray(_lena()[y0:y0 + h, x0:x0 + w])
    raise ValueError(kind)


@lru_cache(maxsize=None)
def argb_image(kind, w, h, seed, plane):
    """int32 ARGB [h*w] of rgb_image, read-only (shared between tests)."""
    a = fo.rgb_to_argb(rgb_image(kind, w, h, seed, plane))
    a.setflags(write=False)
    return a


def case_images(c, first=0):
    """int32 [planes, h*w]: images first .. first + planes - 1 of the case."""
    return np.stack([argb_image(c.kind, c.w, c.h, c.seed, first + p) for p in range(c.planes)])


# ---- references of the fixed-B colour cases -----------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def rgb_reference(w, h, B, wK, n_iso, kind, seed, plane):
    """dict(info float32 [N_r, 5], iso int32 [N_r], qrows int32 [N_r, 5], collage int32 [h*w], decode (rgb uint8 [h, w, 3],
    avgError float32, iterations)) of one image: the oracle's encodeRGB / collage / decodeRGB for n_iso = 1, rgbisomodel for 8."""
    argb = argb_image(kind, w, h, seed, plane)
    if n_iso == 1:
        info = fo.encode_rgb(argb, w, h, B, wK)
        return dict(info=info, iso=np.zeros(len(info), np.int32), qrows=fo.quantise_rgb(info),
                    collage=fo.collage_rgb(argb, w, h, B, wK, info), decode=fo.decode_rgb(fo.write_run_rgb(info, w, h, B, wK)))
    r = rim.encode(argb, w, h, B, wK, 8)
    return dict(info=r["info"], iso=r["iso"], qrows=r["qrows"], collage=rim.collage(argb, w, h, B, wK, r["info"], r["iso"]),
                decode=rim.decode(r["qrows"], r["iso"], w, h, B, wK))


def case_reference(c, plane):
    return rgb_reference(c.w, c.h, c.B, c.wK, c.n_iso, c.kind, c.seed, plane)


# ---- references of the quadtree cases -----------------------------------------------------------------------------------------
def qt_image(c):
    """int32 ARGB [h*w].  S: the S planes cut out of a larger image at (24, 24), so that the 32-pixel tiles of flat and noisy
    levels meet inside the smallest images too (a 16 x 16 image at the origin would be one flat tile)."""
    if c.kind == "S":
        rgb = np.stack([synth.image_s(c.w + 24, c.h + 24, c.seed + 101 * ch)[24:, 24:] for ch in range(3)], axis=-1)
        return fo.rgb_to_argb(np.ascontiguousarray(rgb))
    return argb_image(c.kind, c.w, c.h, c.seed, 0)


@lru_cache(maxsize=None)
def qt_reference(c, encoder):
    """dict(argb, gray (the red channel; grey encoders), cbs (the model's level codebooks, from the CPU reference alone), sse {B:
    int64 [Rh, Rw]}) of one quadtree case through one of QT_ENCODERS."""
    argb = qt_image(c)
    w, h = c.w, c.h
    if encoder.startswith("grey"):
        n_iso = int(encoder[-1])
        gray = np.ascontiguousarray(qr.channels(argb, w, h)[..., 0].astype(np.uint8))
        cbs = qm.codebooks(gray, c.B_max, c.B_min, c.wK, n_iso)
        return dict(argb=argb, gray=gray, n_iso=n_iso, cbs=cbs, sse=qm.level_sse(gray, cbs, c.wK))
    if encoder == "rgb":
        cbs = qr.codebooks(argb, w, h, c.B_max, c.B_min, c.wK)
        return dict(argb=argb, n_iso=1, cbs=cbs, sse=qr.level_sse(argb, w, h, cbs, c.wK))
    n_iso = int(encoder[-1])
    cbs = im.codebooks(argb, w, h, c.B_max, c.B_min, c.wK, n_iso)
    return dict(argb=argb, n_iso=n_iso, cbs=cbs, sse=im.level_sse(argb, w, h, cbs, c.wK))


def qt_leaf_table(c, encoder, tree):
    ref = qt_reference(c, encoder)
    table = qm.leaf_table if encoder.startswith("grey") else qr.leaf_table if encoder == "rgb" else im.leaf_table
    return table(tree, ref["cbs"], c.w)


def qt_boundary(c, sse, B):
    """The boundary block of level B > B_min: (x, y, s, t) with s its SSE, 0 < s < 2^24, and t = float32(s / B^2), so that
    (double) s > (double) t * B * B is an equality missed: the block is a leaf at t and split at nextafter(t, -inf).  Among the
    blocks that the walk reaches at t (every ancestor splits there), the one whose (s, scanline index) is the median; None when
    the level has no such block."""
    v = sse[B]
    cand = []
    for j in np.argsort(v.reshape(-1), kind="stable"):
        s = int(v.reshape(-1)[j])
        if not 0 < s < (1 << 24):
            continue
        y, x = int(j) // v.shape[1] * B, int(j) % v.shape[1] * B
        t = float(np.float32(s / (B * B)))
        A, reached = 2 * B, True
        while A <= c.B_max and reached:
            reached = float(sse[A][y // A, x // A]) > t * A * A
            A *= 2
        if reached:
            cand.append((x, y, s, np.float32(t)))
    return cand[len(cand) // 2] if cand else None
