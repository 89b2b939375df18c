"""numpy model of the grey collage (getBestGeneratedCollage FC:269-300) with the n_iso = 8 extension, and an exact check that
the encoder and the painters mean the same thing by an isometry id.  From the oracle only geometry, pool and index helpers are
taken (fo_geometry, fo_pool, fo_calculate_indices, fo_iso_source); the painting arithmetic and the agreement check are restated
here.  Test infrastructure only.

Why painter_agreement must hold.  For one range block r (rM = sum(r) // n, rem = sum(r) % n) and one domain block D, candidate
isometry kk has kovarianz_kk = sum_pos (r[pos] - rM) (D[src_kk(pos)] - dM) = dots[kk] + C with dots[kk] = sum_pos r[pos] D[src_kk(pos)]
and C the same for every kk: the block's sum and variance do not depend on the order of its pixels.  The reference's error
rem^2 (1 - kov^2 / (rem^2 var)) (FC:655-687) falls as |kov| rises, so the winner k of the scan has the largest |kov| of its domain
block and a = kov_k / var has kov_k's sign: sign(a) (dots[k] - dots[kk]) >= 0 for every kk.  The squared residual of painting
a D[src_kk(pos)] + b over r with the winner's (a, b) depends on kk only through -2 a dots[kk]: the same inequality says that painting
through the winner's own id is at least as good as painting through any other id.  An encoder whose copy_k is r o src_{k^-1} and a
painter that reads D at src_k(pos) satisfy it; if one of them took k = 1 for k = 3 (the only two that are not self-inverse) it
fails wherever dots[1] != dots[3].  Ranges with rem = 0 are skipped: every error is 0 there and candidate (0, 0) wins whatever the
covariances are (FC:677)."""
import ctypes as C

import numpy as np

from oracle import fic_oracle as fo

F = np.float32
_ISO = {}


def iso_table(B):
    """int64 [8, B*B]: the painters read domain position iso_table(B)[k, rx + ry*B] for pixel (rx, ry) (fo_iso_source)."""
    if B not in _ISO:
        L = fo.lib()
        _ISO[B] = np.array([[L.fo_iso_source(k, B, p % B, p // B) for p in range(B * B)] for k in range(8)], np.int64)
    return _ISO[B]


def to_global(w, h, B, wK, idx_local):
    """calculateIndices (FC:853-893), the decoder's own mapping: window-local candidate of every range block -> pool index."""
    data = np.ascontiguousarray(idx_local, np.float32).copy()
    Rw, Rh, Dw, Dh = fo.geometry(w, h, B)
    assert data.size == Rw * Rh
    fo.lib().fo_calculate_indices(data.ctypes.data_as(C.POINTER(C.c_float)), 1, w, h, B, wK)
    return data.astype(np.int32)


def java_f2i(v):
    """Java's (int) cast of float32 values as int64: NaN -> 0, out-of-range values saturate at int32 (JLS 5.1.3)."""
    v = np.asarray(v, np.float64)
    nan = np.isnan(v)
    return np.where(nan, 0, np.clip(np.trunc(np.where(nan, 0.0, v)), -2147483648.0, 2147483647.0)).astype(np.int64)


def blocks(img, B):
    """[Rh*Rw, B*B] pixels of every B x B block, blocks in scanline order, position rx + ry*B."""
    h, w = img.shape
    return img.reshape(h // B, B, w // B, B).transpose(0, 2, 1, 3).reshape(-1, B * B)


def unblock(vals, w, h, B):
    """[Rh*Rw, B*B] -> [h, w]."""
    return vals.reshape(h // B, w // B, B, B).transpose(0, 2, 1, 3).reshape(h, w)


def collage(gray, B, gidx, a, b, iso):
    """The collage of `gray` (uint8 [h, w]) from the unquantised codebook {pool index, a, b, isometry} per range block:
    (ARGB int32 [h*w], v float32 [N_r, B*B]) with v the value before the cast and the clamp.  Pixel pos = rx + ry*B of range
    block j is painted from d = pool[gidx[j]][src_iso[j](rx, ry)] as clamp((int) fl(fl(a[j] * (float) d) + b[j]), 0, 255)."""
    g = np.ascontiguousarray(gray, np.uint8)
    h, w = g.shape
    pix = fo.pool(fo.gray_to_argb(g), w, h, B)[0]
    src = iso_table(B)[np.asarray(iso, np.int64)]                     # [N_r, n]
    d = pix[np.asarray(gidx, np.int64)[:, None], src].astype(F)
    a = np.asarray(a, F)[:, None]
    b = np.asarray(b, F)[:, None]
    with np.errstate(invalid="ignore"):
        v = ((a * d).astype(F) + b).astype(F)                         # one rounding per operation, never fused
    value = np.clip(java_f2i(v), 0, 255).astype(np.uint32)
    out = np.uint32(0xFF000000) | (value << np.uint32(16)) | (value << np.uint32(8)) | value
    return unblock(out, w, h, B).reshape(-1).view(np.int32).copy(), v


def overshoot_image():
    """uint8 [64, 64] whose collage leaves 0..255 on both sides before the clamp at B = 4 (full search and wK = 5) and at B = 8
    with wK = 3.  Left half: a grid of 16 x 32 cells of 2 x 2 pixels, 100 or 110 at random, 4 % of the cells 80 and 4 % 130, so
    the scaled image is the grid itself: low-contrast domain blocks.  Right half: the grid thresholded to 0 / 255 at pixel
    resolution, tiled 2 x 2: range blocks of full contrast with the same pattern, hence |a| = 1 after the clamp of a and values
    past both ends wherever a cell is 80 or 130."""
    rng = np.random.RandomState(3)
    grid = np.where(rng.rand(32, 16) < 0.5, 100, 110)
    u = rng.rand(32, 16)
    grid[u < 0.04] = 80
    grid[u > 0.96] = 130
    left = np.repeat(np.repeat(grid, 2, axis=0), 2, axis=1)
    right = np.tile(np.where(grid < 105, 0, 255), (2, 2))
    return np.concatenate([left, right], axis=1).astype(np.uint8)


def cell_image(size, seed):
    """uint8 [size, size] of 2 x 2-pixel cells with values 60..199: scaleImage returns the cell grid itself, so scaling commutes
    with a rotation of the image by 90 degrees."""
    cells = np.random.RandomState(seed).randint(60, 200, size=(size // 2, size // 2))
    return np.repeat(np.repeat(cells, 2, axis=0), 2, axis=1).astype(np.uint8)


def painter_agreement(gray, B, pool_pix, gidx, a, iso):
    """Exact (int64) check of the module docstring's inequality on one codebook.  pool_pix: [N_d, B*B] integers, the pool the
    codebook was searched in; gidx / a / iso: [N_r].  Returns a dict of counts:
      total                ranges
      used                 ranges with rem != 0 and a finite, non-zero
      violations           used ranges with sign(a) (dots[iso] - dots[kk]) < 0 for some kk
      strict13             used ranges with iso in {1, 3} and sign(a) (dots[iso] - dots[4 - iso]) > 0
      swapped_violations   `violations` with iso in {1, 3} painted as 4 - iso (what a disagreeing painter would do)"""
    g = np.ascontiguousarray(gray, np.uint8)
    n = B * B
    r = blocks(g, B).astype(np.int64)                                 # [N_r, n]
    a = np.asarray(a, F)
    iso = np.asarray(iso, np.int64)
    D = np.asarray(pool_pix).astype(np.int64)[np.asarray(gidx, np.int64)]          # [N_r, n] the winner's domain block
    dots = np.stack([(r * D[:, iso_table(B)[kk]]).sum(axis=1) for kk in range(8)], axis=1)   # [N_r, 8]
    with np.errstate(invalid="ignore"):
        used = (r.sum(axis=1) % n != 0) & np.isfinite(a) & (a != 0)
        sgn = np.where(a > 0, 1, -1).astype(np.int64)
    rows = np.arange(r.shape[0])

    def violating(painted):
        margin = sgn[:, None] * (dots[rows, painted][:, None] - dots)
        return used & (margin < 0).any(axis=1)

    is13 = (iso == 1) | (iso == 3)
    other = np.where(is13, 4 - iso, iso)
    strict = used & is13 & (sgn * (dots[rows, iso] - dots[rows, other]) > 0)
    return {"total": int(r.shape[0]), "used": int(used.sum()), "violations": int(violating(iso).sum()),
            "strict13": int(strict.sum()), "swapped_violations": int(violating(other).sum())}


def check_agreement(c):
    """The conditions every painter-agreement test asks of painter_agreement's counts, on the CPU and on the device: no
    violation; at most 15 % of the ranges skipped; at least 4 ranges whose winner is k = 1 or k = 3 with dots[1] != dots[3], each
    of which a painter that exchanged the two would break."""
    assert c["violations"] == 0
    assert c["total"] - c["used"] <= 0.15 * c["total"]
    assert c["strict13"] >= 4
    assert c["swapped_violations"] >= 4
