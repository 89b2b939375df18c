"""numpy model of the streams that carry an isometry column, on the existing models: the fixed-B
streams of tag 4 (grey) and tag 5 (colour), the colour quadtree with the 8 isometries and its tag-6 stream.  Writers and
readers, the colour collage SSE through an isometry (qtrgbmodel.paint_values on the block permuted by qtmodel.iso_table), the
tag-6 encode (rgbisomodel.encode per level, then qtmodel.split), the decode references at zoom 1, 2, 4 (zoommodel.decode_rows,
rgbisomodel.decode on the zoomed geometry, the per-level leaf loop of zoommodel), hand-built tag-6 cases on the tree of
streammodel.tree and the streams that never converge.  Test infrastructure only."""
import struct
from functools import lru_cache

import numpy as np

import qtmodel as qm
import qtrgbmodel as rm
import rgbisomodel as rim
import streammodel as sm
import zoommodel as zm

FIXED_QW = {4: 3, 5: 5}                     # ints of a quantised row per tag
LEAF_FIELDS = rm.LEAF_FIELDS + ("iso",)


# ---- tags 4 and 5: fixed B -----------------------------------------------------------------------------------------------------
def write_fixed(tag, rows, iso, w, h, B, wK):
    """{tag, w, h, 0, B, wK} then {row, iso} per range block in scanline order, big-endian int32."""
    rows = np.asarray(rows, np.int32).reshape(-1, FIXED_QW[tag])
    body = np.concatenate([rows, np.asarray(iso, np.int32).reshape(-1, 1)], axis=1)
    return struct.pack(">6i", tag, w, h, 0, B, wK) + np.ascontiguousarray(body, ">i4").tobytes()


def read_fixed(run):
    """Parses and checks a tag-4 / tag-5 stream: (dict(tag, w, h, B, wK), rows int32 [N_r, QW], iso int32 [N_r]); ValueError for
    a malformed one."""
    if len(run) < 24:
        raise ValueError("shorter than the header")
    tag, w, h, zero, B, wK = struct.unpack(">6i", run[:24])
    if tag not in FIXED_QW or zero != 0:
        raise ValueError(f"header {tag}, {zero}")
    if B not in (4, 8, 16) or w <= 0 or h <= 0 or w % 2 or h % 2 or w % B or h % B:
        raise ValueError("geometry")
    Rw, Rh, Dw, Dh = w // B, h // B, 2 * (w // B) - 3, 2 * (h // B) - 3
    if Dw < 1 or Dh < 1:
        raise ValueError("geometry")
    if not 1 <= wK <= min(Dw, Dh):
        raise ValueError("window")
    per = FIXED_QW[tag] + 1
    if len(run) != 24 + 4 * per * Rw * Rh:
        raise ValueError("length")
    body = np.frombuffer(run[24:], ">i4").astype(np.int32).reshape(-1, per)
    rows, iso = body[:, :-1].copy(), body[:, -1].copy()
    if ((rows[:, 0] < 0) | (rows[:, 0] >= wK * wK)).any():
        raise ValueError("idx_local outside the window")
    if ((iso < 0) | (iso > 7)).any():
        raise ValueError("isometry")
    return dict(tag=tag, w=w, h=h, B=B, wK=wK), rows, iso


def decode_fixed(run, z=1, avg_error_in=0.0):
    """The decode of a tag-4 / tag-5 stream at zoom z: (gray uint8 [z*h, z*w] or rgb uint8 [z*h, z*w, 3], avgError float32,
    iterations), on the geometry (z*w, z*h, z*B, wK)."""
    hd, rows, iso = read_fixed(run)
    if hd["tag"] == 4:
        return zm.decode_rows(rows, iso, hd["w"], hd["h"], hd["B"], hd["wK"], z, avg_error_in)
    return rim.decode(rows, iso, z * hd["w"], z * hd["h"], z * hd["B"], hd["wK"], avg_error_in)


# ---- tag 6: the colour quadtree with isometries ----------------------------------------------------------------------------------
def paint_values(scaled, B, gi, q, iso):
    """decodeRGB's value at every pixel of the given range blocks through their isometries, int64 [n, B*B, 3]: position i takes
    the value computed from the domain pixel at src_k(i)."""
    v = rm.paint_values(scaled, B, gi, q)
    return v[np.arange(v.shape[0])[:, None], qm.iso_table(B)[np.asarray(iso, np.int64)]]


def collage_sse(orig, B, wK_B, qrows5, iso):
    """int64 [Rh, Rw]: SSE over pixels and channels of every range block's quantised row, painted through its isometry."""
    h, w = orig.shape[:2]
    gi = qm.global_index(w, h, B, wK_B, qrows5[:, 0])
    d = rm.blocks(orig, B) - paint_values(rm.scale_rgb(orig), B, gi, qrows5, iso)
    return (d * d).sum(axis=(1, 2)).reshape(h // B, w // B)


def codebooks(argb, w, h, B_max, B_min, wK=0, n_iso=8):
    """{B: (qrows5 int32 [N_r, 5], iso int32 [N_r])} of every level, from rgbisomodel.encode."""
    out = {}
    for B in qm.levels(B_max, B_min):
        r = rim.encode(argb, w, h, B, qm.level_wk(w, h, B, wK), n_iso)
        out[B] = (r["qrows"], r["iso"].astype(np.int32))
    return out


def level_sse(argb, w, h, cbs, wK=0):
    orig = rm.channels(argb, w, h)
    return {B: collage_sse(orig, B, qm.level_wk(w, h, B, wK), q, k) for B, (q, k) in cbs.items()}


def leaf_table(tree, cbs, w):
    """int32 [n, 9] rows {x, y, B, idx_local, q1, q2, q3, q4, iso} of the leaves."""
    rows = []
    for x, y, B in tree:
        q, k = cbs[B]
        j = (y // B) * (w // B) + x // B
        rows.append((x, y, B, *q[j], k[j]))
    return np.array(rows, np.int32).reshape(-1, 9)


def encode(argb, w, h, B_max, B_min, wK=0, n_iso=8, threshold=float("inf"), cbs=None):
    cbs = cbs if cbs is not None else codebooks(argb, w, h, B_max, B_min, wK, n_iso)
    sse = level_sse(argb, w, h, cbs, wK)
    return leaf_table(qm.split(sse, w, h, B_max, B_min, threshold), cbs, w)


def write_qt(leaves, w, h, B_max, B_min, wK):
    """The tag-6 stream: {6, w, h, 0, B_max, B_min, wK, n} then {B, idx_local, q1, q2, q3, q4, iso} per leaf, big-endian."""
    hdr = np.array([6, w, h, 0, B_max, B_min, wK, len(leaves)], ">i4")
    return hdr.tobytes() + np.ascontiguousarray(np.asarray(leaves, np.int32).reshape(-1, 9)[:, 2:], ">i4").tobytes()


def tag3_twin(run):
    """The tag-3 stream of the same leaves without their isometry column (what a tag-6 stream with a column of zeros must decode
    like)."""
    hd = struct.unpack(">8i", run[:32])
    body = np.frombuffer(run[32:], ">i4").reshape(hd[7], 7)
    return struct.pack(">8i", 3, *hd[1:]) + np.ascontiguousarray(body[:, :6]).tobytes()


def read_qt(run):
    """Parses and checks a tag-6 stream with the checks of qtrgbmodel.read_run: (header dict, leaves int32 [n, 9])."""
    if len(run) < 32:
        raise ValueError("shorter than the header")
    hd = struct.unpack(">8i", run[:32])
    if hd[0] != 6 or hd[3] != 0:
        raise ValueError(f"header {hd[0]}, {hd[3]}")
    n = hd[7]
    if n < 1 or len(run) != 32 + 28 * n:
        raise ValueError("length")
    head, leaves8 = rm.read_run(tag3_twin(run))
    iso = np.frombuffer(run[32:], ">i4").astype(np.int32).reshape(n, 7)[:, 6]
    if ((iso < 0) | (iso > 7)).any():
        raise ValueError("isometry")
    return head, np.concatenate([leaves8, iso[:, None]], axis=1)


def decode_qt(run, z=1, avg_error_in=0.0):
    """The decode of a tag-6 stream at zoom z: (rgb uint8 [z*h, z*w, 3], avgError float32, iterations); the loop of
    zoommodel.decode_rgb_quadtree with every leaf painted through its isometry at side z*B."""
    hd, leaves = read_qt(run)
    lev, w, h = zm._zoomed_levels(hd, leaves, z)
    per = {B: (gi, lv[:, 3:8], lv[:, 8], rr, cc, so) for B, (lv, gi, rr, cc, so) in lev.items()}
    img, avg, it = zm._loop(w, h, per, np.full((h, w, 3), 128, np.int64), rm.scale_rgb, paint_values, avg_error_in)
    return img.astype(np.uint8), avg, it


# ---- hand-built cases -------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def quadtree_case(w, h, wK, seed):
    """A tag-6 stream on the tree, rows, designated rows and pool-corner leaves of streammodel.rgb_quadtree_case, with the
    isometry column of streammodel.grey_quadtree_case: leaf i of a side carries isometry i % 8.  dict(run, w, h, wK, leaves int32
    [n, 9], designated)."""
    c = sm.rgb_quadtree_case(w, h, wK, seed)
    leaves = np.concatenate([c["leaves"], np.zeros((len(c["leaves"]), 1), np.int32)], axis=1)
    for B in sm.SIDES:
        sel = np.nonzero(leaves[:, 2] == B)[0]
        leaves[sel, 8] = np.arange(sel.size) % 8
    return dict(run=write_qt(leaves, w, h, 16, 4, wK), w=w, h=h, wK=wK, leaves=leaves, designated=c["designated"])


@lru_cache(maxsize=None)
def fixed_case(tag, w, h, B, wK, seed):
    """A tag-4 / tag-5 stream from streammodel.fixed_case (tag 0 / 1) of the same arguments, range block j with isometry
    (j + j // Rw) % 8: every isometry in every block row and column.  dict(run, w, h, B, wK (resolved), rows, iso, designated)."""
    c = sm.fixed_case(tag - 4, w, h, B, wK, seed)
    j = np.arange(len(c["rows"]))
    iso = ((j + j // (w // B)) % 8).astype(np.int32)
    return dict(run=write_fixed(tag, c["rows"], iso, w, h, B, c["wK"]), w=w, h=h, B=B, wK=c["wK"], rows=c["rows"], iso=iso,
                designated=c["designated"])


def oscillating(run, seed=7):
    """The recipe of streammodel.oscillating for tags 4, 5, 6: every a replaced by the stream's encoding of -1 and every b drawn
    from 270..330, isometries kept: the loop runs all 50 iterations on the sequential float path."""
    rng = np.random.RandomState(seed)
    tag = struct.unpack(">i", run[:4])[0]
    hdr, per, first = {4: (24, 4, 1), 5: (24, 6, 1), 6: (32, 7, 2)}[tag]
    body = np.frombuffer(run[hdr:], ">i4").astype(np.int64).reshape(-1, per).copy()
    n = body.shape[0]
    if tag == 4:
        body[:, first] = -100
        body[:, first + 1] = rng.randint(270, 331, n)
    else:
        body[:, first] = -1000000
        body[:, first + 1] = rng.randint(270, 331, n) * 100000
        body[:, first + 2] = rng.randint(270, 331, n) * 100000
        body[:, first + 3] = rng.randint(270, 331, n)
    return bytes(run[:hdr]) + body.astype(">i4").tobytes()


# (w, h, wK, seed): the geometries of streammodel.QT_CASES.  The seeds are the first for which every (zoom * side, k != 0) pair
# shows in the decoded pixels at zoom 1, 2 and 4 (test_iso_streams_model.py: zero insensitive pairs); a changed builder may
# need other seeds.
QT_CASES = [(64, 64, 0, 1), (128, 64, 2, 1), (64, 128, 2, 1), (128, 64, 5, 1), (64, 128, 5, 1)]


def oscillators():
    """One non-converging stream per new tag: the fixed-B ones non-square with a window, the quadtree one on the 64 x 64 base
    (zoom 4 in numpy stays quick)."""
    return {"tag4": oscillating(fixed_case(4, 128, 64, 8, 2, 8)["run"]), "tag5": oscillating(fixed_case(5, 128, 64, 8, 2, 18)["run"]),
            "tag6": oscillating(quadtree_case(*QT_CASES[0])["run"])}


@lru_cache(maxsize=None)
def reference(run, z, avg_error_in=0.0):
    """(pixels, avgError, iterations) of the model of the stream's tag at zoom z, computed once per process."""
    tag = struct.unpack(">i", run[:4])[0]
    return (decode_qt if tag == 6 else decode_fixed)(run, z, avg_error_in)
