"""numpy model of the quadtree (variable block size) grey codec: per-level codebooks from the oracle,
collage SSE of the quantised rows, the top-down split, leaf order, the tag-2 stream and the decoder loop with Java's float
arithmetic (float32 op by op, the avgError sum as one sequential np.add.accumulate).  Built on the oracle's encode_gray /
quantise_gray / pool / calculateIndices and fo_iso_source; test infrastructure only."""
import ctypes as C
import struct

import numpy as np

from oracle import fic_oracle as fo

LEAF_FIELDS = ("x", "y", "B", "idx_local", "qa", "qb", "iso")


def levels(B_max, B_min):
    return [B for B in (16, 8, 4) if B_min <= B <= B_max]


def level_wk(w, h, B, wK):
    """wK = 0: full search at every level (wK_B = Dw_B), else the same wK everywhere."""
    return fo.geometry(w, h, B)[2] if wK == 0 else wK


_ISO = {}


def iso_table(B):
    """int [8, B*B]: position x + y*B of isometry k's output reads domain position iso_table(B)[k, x + y*B] (fo_iso_source)."""
    if B not in _ISO:
        L = fo.lib()
        _ISO[B] = np.array([[L.fo_iso_source(k, B, p % B, p // B) for p in range(B * B)] for k in range(8)], np.int64)
    return _ISO[B]


def global_index(w, h, B, wK_B, idx_local):
    """calculateIndices (FC:853-893): window-local candidate of every range block of one level -> pool index."""
    info = np.zeros((idx_local.size, 3), np.float32)
    info[:, 0] = idx_local
    fo.lib().fo_calculate_indices(info.ctypes.data_as(C.POINTER(C.c_float)), 3, w, h, B, wK_B)
    return info[:, 0].astype(np.int64)


def codebooks(gray, B_max, B_min, wK=0, n_iso=1):
    """{B: (qrows int32 [N_r, 3], iso int32 [N_r])} of every level, from the oracle's encoder."""
    h, w = gray.shape
    argb = fo.gray_to_argb(gray)
    out = {}
    for B in levels(B_max, B_min):
        r = fo.encode_gray(argb, w, h, B, level_wk(w, h, B, wK), n_iso)
        out[B] = (fo.quantise_gray(r["info"]), r["iso"].astype(np.int32))
    return out


def paint_values(img, B, gi, qa, qb, iso):
    """The decoder's value at every pixel of the given range blocks, [n, B*B] (position x + y*B): a = (float) qa / 100f,
    b = (float) qb, value = clamp((int) fl(fl(a * d) + b)), d the domain pixel of pool block gi through isometry iso, the pool
    built from `img` (FC:382-402)."""
    h, w = img.shape
    pix = fo.pool(fo.gray_to_argb(img), w, h, B)[0]
    d = pix[gi[:, None], iso_table(B)[iso]].astype(np.float32)
    a = (np.asarray(qa).astype(np.float32) / np.float32(100.0))[:, None]
    b = np.asarray(qb).astype(np.float32)[:, None]
    v = (a * d).astype(np.float32) + b                      # two roundings, never fused
    return np.clip(np.trunc(v).astype(np.int64), 0, 255)


def blocks(img, B):
    """[Rh*Rw, B*B] pixels of every B x B block, scanline order of blocks, position x + y*B."""
    h, w = img.shape
    return img.reshape(h // B, B, w // B, B).transpose(0, 2, 1, 3).reshape(-1, B * B).astype(np.int64)


def collage_sse(gray, B, wK_B, qrows, iso):
    """int64 [Rh, Rw]: SSE of every range block's quantised row against the original image."""
    h, w = gray.shape
    gi = global_index(w, h, B, wK_B, qrows[:, 0])
    v = paint_values(gray, B, gi, qrows[:, 1], qrows[:, 2], iso)
    d = blocks(gray, B) - v
    return (d * d).sum(axis=1).reshape(h // B, w // B)


def level_sse(gray, cbs, wK=0):
    h, w = gray.shape
    return {B: collage_sse(gray, B, level_wk(w, h, B, wK), q, k) for B, (q, k) in cbs.items()}


def split(sse, w, h, B_max, B_min, threshold):
    """Leaves (x, y, B) in stream order: split a block iff B > B_min and (double) SSE_B > (double) threshold * B * B."""
    t = float(np.float32(threshold))
    out = []

    def visit(x, y, B):
        if B > B_min and float(sse[B][y // B, x // B]) > t * B * B:
            hb = B // 2
            for dx, dy in ((0, 0), (hb, 0), (0, hb), (hb, hb)):
                visit(x + dx, y + dy, hb)
        else:
            out.append((x, y, B))

    for y in range(0, h, B_max):
        for x in range(0, w, B_max):
            visit(x, y, B_max)
    return out


def leaf_table(tree, cbs, w):
    """int32 [n, 7] rows {x, y, B, idx_local, qa, qb, iso} of the leaves."""
    rows = []
    for x, y, B in tree:
        q, k = cbs[B]
        j = (y // B) * (w // B) + x // B
        rows.append((x, y, B, q[j, 0], q[j, 1], q[j, 2], k[j]))
    return np.array(rows, np.int32).reshape(-1, 7)


def encode(gray, B_max, B_min, wK=0, n_iso=1, threshold=float("inf"), cbs=None):
    h, w = gray.shape
    cbs = cbs if cbs is not None else codebooks(gray, B_max, B_min, wK, n_iso)
    sse = level_sse(gray, cbs, wK)
    return leaf_table(split(sse, w, h, B_max, B_min, threshold), cbs, w)


def write_run(leaves, w, h, B_max, B_min, wK, n_iso):
    """The tag-2 stream: {2, w, h, B_max, B_min, wK, n_iso, n} then {B, idx_local, qa, qb[, iso]} per leaf, big-endian."""
    cols = [2, 3, 4, 5] + ([6] if n_iso == 8 else [])
    hdr = np.array([2, w, h, B_max, B_min, wK, n_iso, len(leaves)], ">i4")
    return hdr.tobytes() + np.ascontiguousarray(np.asarray(leaves, np.int32)[:, cols], ">i4").tobytes()


def read_run(run):
    """Parses and checks a tag-2 stream.  Returns (header dict, leaves int32 [n, 7]); ValueError for a malformed stream."""
    if len(run) < 32:
        raise ValueError("shorter than the header")
    tag, w, h, B_max, B_min, wK, n_iso, n = struct.unpack(">8i", run[:32])
    if tag != 2:
        raise ValueError(f"tag {tag}")
    if B_max not in (8, 16) or B_min not in (4, 8) or B_min >= B_max or n_iso not in (1, 8):
        raise ValueError("levels / n_iso")
    if w <= 0 or h <= 0 or w % B_max or h % B_max or wK < 0 or (wK == 0 and w != h):
        raise ValueError("geometry")
    per = 5 if n_iso == 8 else 4
    if n < 1 or len(run) != 32 + 4 * per * n:
        raise ValueError("length")
    body = np.frombuffer(run[32:], ">i4").astype(np.int32).reshape(n, per)
    wk = {B: level_wk(w, h, B, wK) for B in levels(B_max, B_min)}
    tree, i = [], 0

    def visit(x, y, B):
        nonlocal i
        if i >= n:
            raise ValueError("too few leaves")
        b = int(body[i, 0])
        if b == B:
            tree.append((x, y, B))
            i += 1
        elif b < B and B > B_min:
            hb = B // 2
            for dx, dy in ((0, 0), (hb, 0), (0, hb), (hb, hb)):
                visit(x + dx, y + dy, hb)
        else:
            raise ValueError(f"leaf {i}: B={b} does not tile")

    for y in range(0, h, B_max):
        for x in range(0, w, B_max):
            visit(x, y, B_max)
    if i != n:
        raise ValueError("too many leaves")
    leaves = np.zeros((n, 7), np.int32)
    leaves[:, :3] = np.array(tree, np.int32)
    leaves[:, 3:3 + per - 1] = body[:, 1:]
    if ((leaves[:, 3] < 0) | (leaves[:, 3] >= np.array([wk[b] ** 2 for b in leaves[:, 2]]))).any():
        raise ValueError("idx_local outside the window")
    if ((leaves[:, 6] < 0) | (leaves[:, 6] >= n_iso)).any():
        raise ValueError("isometry")
    return dict(w=w, h=h, B_max=B_max, B_min=B_min, wK=wK, n_iso=n_iso), leaves


def decode(run, avg_error_in=0.0):
    """The decoder loop of decodeGreyScale (FC:356-421) over the leaves: grey 128, at most 50 iterations, each one painting
    every leaf from its own level's pool of the image before the iteration; the squared changes in leaf order (pixel rows
    within a leaf) summed like Java's `avgError += (float) d` (FC:407).  Returns (gray uint8 [H,W], avgError float32, iterations)."""
    hd, leaves = read_run(run)
    w, h, B_max, B_min = hd["w"], hd["h"], hd["B_max"], hd["B_min"]
    Bs = leaves[:, 2].astype(np.int64)
    offs = np.concatenate([[0], np.cumsum(Bs * Bs)[:-1]])
    per = {}
    for B in levels(B_max, B_min):
        sel = np.nonzero(Bs == B)[0]
        if sel.size == 0:
            continue
        lv = leaves[sel]
        Rw = w // B
        j = (lv[:, 1] // B) * Rw + lv[:, 0] // B
        loc = np.zeros((h // B) * Rw, np.int32)
        loc[j] = lv[:, 3]
        gi = global_index(w, h, B, level_wk(w, h, B, hd["wK"]), loc)[j]
        pos = np.arange(B * B)
        rr = lv[:, 1][:, None] + pos // B
        cc = lv[:, 0][:, None] + pos % B
        per[B] = (gi, lv[:, 4], lv[:, 5], lv[:, 6], rr, cc, offs[sel][:, None] + pos)
    img = np.full((h, w), 128, np.uint8)
    avg = np.float32(avg_error_in)
    iters = 0
    for counter in range(50):
        vals = {B: paint_values(img, B, gi, qa, qb, k) for B, (gi, qa, qb, k, _, _, _) in per.items()}   # pools before the paint
        sq = np.zeros(w * h, np.int64)
        for B, (_, _, _, _, rr, cc, so) in per.items():
            d = img[rr, cc].astype(np.int64) - vals[B]
            sq[so] = d * d
            img[rr, cc] = vals[B]
        acc = np.add.accumulate(np.concatenate([[avg], sq.astype(np.float32)]).astype(np.float32), dtype=np.float32)
        avg = np.float32(acc[-1] / np.float32(w * h))
        iters = counter + 1
        if avg < 1:
            break
        if counter != 49:
            avg = np.float32(0.0)
    return img, np.float32(avg), iters
