"""Hand-built decoder inputs: legal streams of all four tags whose tree, isometry column, domain
indices and (a, b) rows are fixed by construction instead of being whatever an encoder chose, so that a decoder test reaches
every (block side, isometry) pair, the blocks at the pool's corners, both sides of the clamp, Java's float-to-int saturation
and the 50-iteration sequential avgError path on purpose.  numpy plus the existing models; no GPU code; the only randomness is a
np.random.RandomState with a fixed seed.  Test infrastructure only.

The tree of a quadtree case (top blocks of side 16 in scanline order, tx / ty the block's column / row):
  * the four corner blocks are split: top left and bottom right deep -- two of the 8-quadrants, the corner-most among them,
    split again into 4-leaves, the other two 8-leaves --, top right and bottom left deep as well with a search window
    (wK > 0) and four 8-leaves under full search; their horizontal neighbours stay leaves of side 16;
  * on more than 4 x 4 top blocks, (tx + 3 ty) % 8 == 2 -> a deep block ({0, 3} or {1, 2} split in turn) and
    (tx + 3 ty) % 8 in {5, 7} -> four 8-leaves: blocks of different depth lie on diagonals;
  * everything else stays a leaf of side 16.
A 32 x 32 domain region always spans leaves with different rows, and the pool's corner blocks of every level lie in split
corner blocks, so none of them is flat after the first paint.  With a window, the leaves in and next to a corner block share
the window of the level's corner range block (getDomainBlockIndex folds row / column 0 onto 1 and the last onto the one
before, FC:516-545), so a leaf of every side can carry the window corner that resolves to the pool's corner.  On 64 x 64
that leaves the minimum the coverage needs: 12 leaves of side 16, 12 of side 8, 16 of side 4."""
import struct
from functools import lru_cache

import numpy as np

import qtmodel as qm
import qtrgbmodel as rm
import rgbisomodel as rim
import zoommodel as zm
from oracle import fic_oracle as fo

INT_MAX, INT_MIN = 2147483647, -2147483648
SIDES = (16, 8, 4)

# Designated grey rows (qa, qb).  "all_0", "all_255" and "max_max" paint a constant whatever the domain block holds.
GREY_ROWS = {
    "all_0": (0, -5),                      # b below the range: the whole leaf 0
    "all_255": (0, 300),                   # b above the range: the whole leaf 255
    "low": (90, -200),                     # 0.9 d - 200: below 0 up to d = 222, at most 29
    "both": (-150, 400),                   # 400 - 1.5 d: 255 up to d = 96, then down to 17
    "max_min": (INT_MAX, INT_MIN),         # fl(2^31 / 100) d - 2^31: below 0 for d < 100, 0 at d = 100, far above 255 beyond
    "min_max": (INT_MIN, INT_MAX),         # the mirror image: (int) saturates at INT_MAX for small d
    "max_max": (INT_MAX, INT_MAX),         # >= 2^31 everywhere: (int) saturates, the clamp gives 255
}
GREY_CONSTANT = {"all_0": 0, "all_255": 255, "max_max": 255}

# Designated colour rows (q1, q2, q3, q4): a = q1 / 1e6, bR = q2 / 1e5, bG = q3 / 1e5, bB = q4.  rgb_*: a = 0 and one channel
# below 0, one above 255, one inside, in the three cyclic orders; then the saturation rows.
RGB_ROWS = {
    "rgb_0_255_in": (0, -5 * 100000, 300 * 100000, 100),
    "rgb_in_0_255": (0, 100 * 100000, -5 * 100000, 300),
    "rgb_255_in_0": (0, 300 * 100000, 100 * 100000, -5),
    "max_min": (INT_MAX, INT_MIN, INT_MIN, INT_MIN),
    "min_max": (INT_MIN, INT_MAX, INT_MAX, INT_MAX),
    "max_max": (INT_MAX, INT_MAX, INT_MAX, INT_MAX),
}
RGB_CONSTANT = {"rgb_0_255_in": (0, 255, 100), "rgb_in_0_255": (100, 0, 255), "rgb_255_in_0": (255, 100, 0)}


# ---- the pool's corners -------------------------------------------------------------------------------------------------------
def pool_corners(w, h, B):
    """Pool indices 0, Dw-1, Dw*(Dh-1), Nd-1 of level B."""
    _, _, Dw, Dh = fo.geometry(w, h, B)
    return [0, Dw - 1, Dw * (Dh - 1), Dw * Dh - 1]


def window_table(w, h, B, wK_B):
    """int64 [N_r, wK_B^2]: the pool index of window candidate c of every range block of level B."""
    return rim.window_globals(w, h, B, wK_B)


def corner_targets(w, h, B, wK):
    """Per pool corner (top-left, top-right, bottom-left, bottom-right): (range block j at that image corner, the window-local
    index of the window's own corner, the pool index it resolves to).  Full search: the pool's corners themselves.  With a
    window the resolved index is the pool's corner where the window reaches it (wK >= 5 on these geometries) and the farthest
    block any window reaches otherwise: the window of the last range column starts at Dw - 3 - wK / 2 (FC:84-100, 516-545)."""
    Rw, Rh, Dw, Dh = fo.geometry(w, h, B)
    wk = qm.level_wk(w, h, B, wK)
    G = window_table(w, h, B, wk)
    js = [0, Rw - 1, Rw * (Rh - 1), Rw * Rh - 1]
    cs = [0, wk - 1, wk * (wk - 1), wk * wk - 1]
    return [(j, c, int(G[j, c])) for j, c in zip(js, cs)]


# ---- the tree ---------------------------------------------------------------------------------------------------------------
def tree(w, h, wK):
    """Leaves (x, y, B) in stream order (module docstring)."""
    tw, th = w // 16, h // 16
    out, deep = [], 0
    for ty in range(th):
        for tx in range(tw):
            x, y = 16 * tx, 16 * ty
            m = (tx + 3 * ty) % 8 if tw * th > 16 else 0
            kind, split = ("deep", None) if m == 2 else (("eights", None) if m in (5, 7) else ("leaf", None))
            if ty in (0, th - 1):
                if tx in (0, tw - 1):
                    q = (1 if tx else 0) + (2 if ty else 0)
                    kind, split = ("deep", {q, 3 - q}) if wK > 0 or q in (0, 3) else ("eights", None)
                elif tx in (1, tw - 2):
                    kind = "leaf"
            if kind == "leaf":
                out.append((x, y, 16))
                continue
            if kind == "deep" and split is None:
                split = {0, 3} if deep % 2 else {1, 2}
                deep += 1
            for q, (dx, dy) in enumerate(((0, 0), (8, 0), (0, 8), (8, 8))):
                if kind == "deep" and q in split:
                    out.extend((x + dx + ex, y + dy + ey, 4) for ex, ey in ((0, 0), (4, 0), (0, 4), (4, 4)))
                else:
                    out.append((x + dx, y + dy, 8))
    return out


def _designated_slots(n):
    """{name: position among the n leaves of one side} for the seven grey designated rows.  The isometry of leaf i of a side is
    i % 8.  From 15 leaves on the rows sit on leaves 0 and 8..13, so leaves 1..7 -- one per isometry k != 0 -- keep rows from
    the generator.  With 12..14 leaves (sides 16 and 8 of a 64 x 64 image) seven designated and seven free leaves do not fit:
    the rows that still depend on the domain block ("both", "low", "max_min", "min_max") take the only leaves of k = 2 and k = 1."""
    assert n >= 12
    if n >= 15:
        order = ["all_0", "all_255", "low", "both", "max_min", "min_max", "max_max"]
        return dict(zip(order, [0, 8, 9, 10, 11, 12, 13]))
    return {"all_0": 0, "max_min": 1, "both": 2, "all_255": 8, "min_max": 9, "low": 10, "max_max": 11}


def _assign_corners(w, h, wK, xyB, idx, free):
    """Writes, per side, the window-local index that resolves to each pool corner into a leaf that shares the window of that
    corner's range block (a leaf from `free` where there is one)."""
    for B in SIDES:
        wk = qm.level_wk(w, h, B, wK)
        G = window_table(w, h, B, wk)
        Rw = w // B
        used = set()
        for j, c, _ in corner_targets(w, h, B, wK):
            cand = [i for i, (x, y, b) in enumerate(xyB)
                    if b == B and i not in used and (wK == 0 or (G[(y // B) * Rw + x // B] == G[j]).all())]
            assert cand, (w, h, wK, B, j)
            pick = [i for i in cand if i in free] or cand
            i = pick[0] if j < Rw else pick[-1]                       # leaves near the image corner concerned
            used.add(i)
            idx[i] = c if wK else int(G[j, c])


def _case(w, h, wK, seed, colour):
    rng = np.random.RandomState(seed)
    xyB = tree(w, h, wK)
    n = len(xyB)
    rows = GREY_ROWS if not colour else RGB_ROWS
    leaves = np.zeros((n, 8 if colour else 7), np.int32)
    leaves[:, :3] = np.array(xyB, np.int32)
    sides = leaves[:, 2]
    designated = {}
    for B in SIDES:
        sel = np.nonzero(sides == B)[0]
        wk = qm.level_wk(w, h, B, wK)
        leaves[sel, 3] = rng.randint(0, wk * wk, sel.size)
        if colour:
            leaves[sel, 4] = rng.randint(-950000, 950001, sel.size)
            leaves[sel, 5] = rng.randint(-40, 301, sel.size) * 100000 + rng.randint(0, 100000, sel.size)
            leaves[sel, 6] = rng.randint(-40, 301, sel.size) * 100000 + rng.randint(0, 100000, sel.size)
            leaves[sel, 7] = rng.randint(-40, 301, sel.size)
            slots = dict(zip(rows, [0, 8, 9, 10, 11, 2]))
        else:
            leaves[sel, 4] = rng.randint(-95, 96, sel.size)
            leaves[sel, 5] = rng.randint(-40, 301, sel.size)
            leaves[sel, 6] = np.arange(sel.size) % 8
            slots = _designated_slots(sel.size)
        for name, s in slots.items():
            leaves[sel[s], 4:4 + len(rows[name])] = rows[name]
            designated[(B, name)] = int(sel[s])
    idx = leaves[:, 3].copy()
    _assign_corners(w, h, wK, xyB, idx, set(range(n)) - set(designated.values()))
    leaves[:, 3] = idx
    run = rm.write_run(leaves, w, h, 16, 4, wK) if colour else qm.write_run(leaves, w, h, 16, 4, wK, 8)
    return dict(run=run, w=w, h=h, wK=wK, leaves=leaves, designated=designated)


@lru_cache(maxsize=None)
def grey_quadtree_case(w, h, wK, seed):
    """A tag-2 stream (B_max = 16, B_min = 4, n_iso = 8): dict(run, w, h, wK, leaves int32 [n, 7] {x, y, B, idx_local, qa, qb,
    iso}, designated {(side, name of GREY_ROWS): leaf})."""
    return _case(w, h, wK, seed, False)


@lru_cache(maxsize=None)
def rgb_quadtree_case(w, h, wK, seed):
    """The same tree and index rule as a tag-3 stream: leaves int32 [n, 8] {x, y, B, idx_local, q1, q2, q3, q4}, designated
    rows of RGB_ROWS."""
    return _case(w, h, wK, seed, True)


def resolved_indices(case, B):
    """The pool index of every leaf of side B of a quadtree case."""
    w, h, lv = case["w"], case["h"], case["leaves"]
    lv = lv[lv[:, 2] == B]
    Rw = w // B
    j = (lv[:, 1] // B) * Rw + lv[:, 0] // B
    loc = np.zeros((h // B) * Rw, np.int32)
    loc[j] = lv[:, 3]
    return qm.global_index(w, h, B, qm.level_wk(w, h, B, case["wK"]), loc)[j]


# ---- fixed-B streams --------------------------------------------------------------------------------------------------------
def fixed_positions(Rw, Rh):
    """Range blocks (bx, by) for the designated rows: image corners, the four edges, the interior."""
    return [(0, 0), (Rw // 2, 0), (Rw - 1, Rh // 2), (Rw // 2, Rh // 2), (0, Rh // 2), (Rw // 2 - 1, Rh - 1), (Rw - 1, Rh - 1)]


@lru_cache(maxsize=None)
def fixed_case(tag, w, h, B, wK, seed):
    """A tag-0 (grey, rows {idx_local, qa, qb}) or tag-1 (colour, rows {idx_local, q1, q2, q3, q4}) stream of zm.fixed_run with
    the designated rows at fixed_positions and the pool-corner rule on the four corner range blocks.  wK = 0: full search.
    dict(run, w, h, B, wK (resolved), rows, designated {name: range block})."""
    rng = np.random.RandomState(seed)
    Rw, Rh, Dw, Dh = fo.geometry(w, h, B)
    wk = qm.level_wk(w, h, B, wK)
    nr = Rw * Rh
    named = RGB_ROWS if tag else GREY_ROWS
    rows = np.zeros((nr, 5 if tag else 3), np.int32)
    rows[:, 0] = rng.randint(0, wk * wk, nr)
    if tag:
        rows[:, 1] = rng.randint(-950000, 950001, nr)
        rows[:, 2] = rng.randint(-40, 301, nr) * 100000 + rng.randint(0, 100000, nr)
        rows[:, 3] = rng.randint(-40, 301, nr) * 100000 + rng.randint(0, 100000, nr)
        rows[:, 4] = rng.randint(-40, 301, nr)
    else:
        rows[:, 1] = rng.randint(-95, 96, nr)
        rows[:, 2] = rng.randint(-40, 301, nr)
    designated = {}
    for name, (bx, by) in zip(named, fixed_positions(Rw, Rh)):
        rows[by * Rw + bx, 1:] = named[name]
        designated[name] = by * Rw + bx
    for j, c, _ in corner_targets(w, h, B, wK):
        rows[j, 0] = c
    return dict(run=zm.fixed_run(tag, rows, w, h, B, wk), w=w, h=h, B=B, wK=wk, rows=rows, designated=designated)


# ---- streams that never converge --------------------------------------------------------------------------------------------
def oscillating(run, seed=7):
    """The same stream with every a replaced by the stream's encoding of -1 and every b drawn from 270..330: x -> b - x flips
    the image for ever, every iteration's sum of squares is far above 2^24 and the loop runs all 50 iterations on the
    sequential float path.  Tags 0..3."""
    rng = np.random.RandomState(seed)
    tag = struct.unpack(">i", run[:4])[0]
    hdr = 20 if tag in (0, 1) else 32
    per, first = {0: (3, 1), 1: (5, 1), 3: (6, 2)}.get(tag, (None, 2))
    if tag == 2:
        per = 5 if struct.unpack(">i", run[24:28])[0] == 8 else 4
    body = np.frombuffer(run[hdr:], ">i4").astype(np.int64).reshape(-1, per).copy()
    n = body.shape[0]
    if tag in (0, 2):
        body[:, first] = -100
        body[:, first + 1] = rng.randint(270, 331, n)
    else:
        body[:, first] = -1000000
        body[:, first + 1] = rng.randint(270, 331, n) * 100000
        body[:, first + 2] = rng.randint(270, 331, n) * 100000
        body[:, first + 3] = rng.randint(270, 331, n)
    return bytes(run[:hdr]) + body.astype(">i4").tobytes()


# ---- the committed cases ---------------------------------------------------------------------------------------------------------
# (w, h, wK, seed).  64 x 64 full search and the two non-square bases with the window of 2 x 2; wK = 2 never reaches the last
# two pool columns / rows (streammodel.corner_targets), so the non-square bases come with wK = 5 as well, where the windows
# of the corner blocks end at the pool's corners.  The seeds are the first for which every (zoom * side, k != 0) pair shows in
# the decoded pixels (test_decode_streams_model.py: zero insensitive pairs); a changed builder may need other seeds.
QT_CASES = [(64, 64, 0, 10), (128, 64, 2, 2), (64, 128, 2, 2), (128, 64, 5, 1), (64, 128, 5, 1)]
FIXED_CASES = [(tag, w, h, B, wK, 10 * tag + B) for tag in (0, 1) for B in (4, 8, 16) for w, h, wK in ((64, 64, 0), (128, 64, 2))]


def oscillators():
    """The four tags' non-converging streams: the quadtree ones on the 64 x 64 base (zoom 4 in numpy stays quick) and on a
    non-square one, the fixed-B ones non-square with a window."""
    return {"tag0": oscillating(fixed_case(0, 128, 64, 8, 2, 8)["run"]), "tag1": oscillating(fixed_case(1, 128, 64, 8, 2, 18)["run"]),
            "tag2": oscillating(grey_quadtree_case(*QT_CASES[0])["run"]), "tag3": oscillating(rgb_quadtree_case(*QT_CASES[0])["run"]),
            "tag2_non_square": oscillating(grey_quadtree_case(*QT_CASES[2])["run"])}


# ---- the references, computed once per process ---------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def reference(run, z, avg_error_in=0.0):
    """(pixels, avgError, iterations) of the reference model of the stream's tag at zoom z."""
    tag = struct.unpack(">i", run[:4])[0]
    fn = (zm.decode_gray, zm.decode_rgb, zm.decode_quadtree, zm.decode_rgb_quadtree)[tag]
    return fn(run, z, avg_error_in)


# ---- images on which an n_iso = 8 encoder chooses every isometry ------------------------------------------------------------------
def _tile(rng, B):
    """An asymmetric 2B x 2B tile: a diagonal ramp, a bright bar along one edge and a bright corner, a little noise."""
    y, x = np.mgrid[0:2 * B, 0:2 * B]
    t = 40.0 + 50.0 * x / (2 * B) + 90.0 * (y / (2 * B)) ** 2
    t[: B // 2, :] += 60
    t[:, : B // 4 + 1] -= 35
    t[B:, B + B // 2:] += 45
    return np.clip(t + rng.randint(-6, 7, t.shape), 0, 255).astype(np.uint8)


@lru_cache(maxsize=None)
def iso_tile_image(B, size):
    """uint8 [size, size]: noise, the tile at the top left (one domain block after scaling) and, on a grid with noise between
    them, eight range blocks 0.75 * (isometry k of the scaled tile) + 20: block k matches the tile's domain block exactly under
    isometry k only."""
    rng = np.random.RandomState(100 + B)
    img = rng.randint(0, 256, (size, size)).astype(np.uint8)
    img[:2 * B, :2 * B] = _tile(rng, B)
    d = fo.pool(fo.gray_to_argb(img), size, size, B)[0][0]                       # pool block 0 = the scaled tile
    T = qm.iso_table(B)
    for k in range(8):
        bx, by = 3 + 2 * (k % 2), 2 * (k // 2) if size // B >= 8 else k // 2
        v = np.trunc(np.float32(0.75) * d[T[k]].astype(np.float32) + np.float32(20)).astype(np.uint8).reshape(B, B)
        img[by * B:(by + 1) * B, bx * B:(bx + 1) * B] = v
    return img


@lru_cache(maxsize=None)
def iso_tile_image_rgb(B, size):
    """uint8 [size, size, 3]: the same layout in colour, the three channels of a range copy with their own offsets."""
    rng = np.random.RandomState(200 + B)
    img = rng.randint(0, 256, (size, size, 3)).astype(np.uint8)
    for c in range(3):
        img[:2 * B, :2 * B, c] = np.roll(_tile(rng, B), 3 * c, axis=1) if c else _tile(rng, B)
    d = rm.scale_rgb(img.astype(np.int64))[:B, :B].reshape(B * B, 3)
    T = qm.iso_table(B)
    for k in range(8):
        bx, by = 3 + 2 * (k % 2), 2 * (k // 2) if size // B >= 8 else k // 2
        v = np.trunc(np.float32(0.75) * d[T[k]].astype(np.float32) + np.array([20, 35, 5], np.float32)).astype(np.uint8)
        img[by * B:(by + 1) * B, bx * B:(bx + 1) * B] = v.reshape(B, B, 3)
    return img
