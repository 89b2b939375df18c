"""numpy model of the quadtree (variable block size) joint-RGB codec: per-level codebooks from the
oracle's encodeRGB, scaleImageRGB with its quirks, decodeRGB's float paint of quantised rows, the collage SSE over three
channels, the top-down split, leaf order, the tag-3 stream and the decoder loop with Java's float arithmetic (float32 op by
op, the avgError sum as one sequential np.add.accumulate).  Reuses qtmodel's levels, window resolution and split; test
infrastructure only."""
import struct

import numpy as np

import qtmodel as qm
from oracle import fic_oracle as fo

LEAF_FIELDS = ("x", "y", "B", "idx_local", "q1", "q2", "q3", "q4")
levels = qm.levels
level_wk = qm.level_wk
split = qm.split


def channels(argb, w, h):
    """int64 [h, w, 3] (R, G, B) of packed ARGB pixels ([h*w] or [h, w])."""
    u = np.asarray(argb).astype(np.int64).reshape(h, w) & 0xFFFFFFFF
    return np.stack([(u >> 16) & 0xFF, (u >> 8) & 0xFF, u & 0xFF], axis=-1)


def pack(rgb):
    """int32 ARGB [h, w] with alpha 255 of int [h, w, 3]."""
    c = np.asarray(rgb).astype(np.uint32)
    return (0xFF000000 | (c[..., 0] << 16) | (c[..., 1] << 8) | c[..., 2]).astype(np.uint32).view(np.int32)


def scale_rgb(img):
    """scaleImageRGB (FC:901-962) of int [H, W, 3], W and H even: per channel (p(x,y) + p(x+1,y) + p(x,y+1) + t) / 4 with
    t = 128 where x + 1 >= image.height (the reference compares x with the height) and t = p(x,y+1) again elsewhere: the
    (x, y+1) pixel is added twice and (x+1, y+1) never."""
    h, w = img.shape[:2]
    p00, p10, p01 = img[0::2, 0::2], img[0::2, 1::2], img[1::2, 0::2]
    x = np.arange(0, w, 2)
    fourth = np.where((x + 1 >= h)[None, :, None], 128, p01)
    return (p00 + p10 + p01 + fourth) // 4


def codebooks(argb, w, h, B_max, B_min, wK=0, only=None):
    """{B: qrows5 int32 [N_r, 5]} of every level (or of the levels in `only`), from the oracle's encodeRGB."""
    a = np.ascontiguousarray(argb, np.int32).reshape(-1)
    return {B: fo.quantise_rgb(fo.encode_rgb(a, w, h, B, level_wk(w, h, B, wK)))
            for B in levels(B_max, B_min) if only is None or B in only}


def paint_values(scaled, B, gi, q):
    """decodeRGB's value at every pixel of the given range blocks, int64 [n, B*B, 3] (position x + y*B): a = (float) q1 / 1e6f,
    bR = (float) q2 / 1e5f, bG = (float) q3 / 1e5f, bB = (float) q4, value_c = clamp((int) fl(fl(a * d_c) + b_c)), d the
    pixel of pool block gi in the scaled image, origin (c * B/4, r * B/4) (FC:446-450, 477-488)."""
    Ws = scaled.shape[1]
    Dw = 2 * (2 * Ws // B) - 3
    ab = B // 4
    gi = np.asarray(gi, np.int64)
    pos = np.arange(B * B)
    rr = (gi // Dw * ab)[:, None] + pos // B
    cc = (gi % Dw * ab)[:, None] + pos % B
    d = scaled[rr, cc].astype(np.float32)                                     # [n, B*B, 3]
    q = np.asarray(q, np.int32).reshape(-1, 5)
    a = q[:, 1].astype(np.float32) / np.float32(1e6)
    b = np.stack([q[:, 2].astype(np.float32) / np.float32(1e5), q[:, 3].astype(np.float32) / np.float32(1e5),
                  q[:, 4].astype(np.float32)], axis=1)
    v = (a[:, None, None] * d).astype(np.float32) + b[:, None, :]            # two roundings, never fused
    return np.clip(np.trunc(v).astype(np.int64), 0, 255)


def blocks(img, B):
    """[Rh*Rw, B*B, 3] pixels of every B x B block of int [H, W, 3], blocks in scanline order, position x + y*B."""
    h, w = img.shape[:2]
    return img.reshape(h // B, B, w // B, B, 3).transpose(0, 2, 1, 3, 4).reshape(-1, B * B, 3).astype(np.int64)


def collage_sse(orig, B, wK_B, qrows5):
    """int64 [Rh, Rw]: SSE over pixels and channels of every range block's quantised row against the original."""
    h, w = orig.shape[:2]
    gi = qm.global_index(w, h, B, wK_B, qrows5[:, 0])
    d = blocks(orig, B) - paint_values(scale_rgb(orig), B, gi, qrows5)
    return (d * d).sum(axis=(1, 2)).reshape(h // B, w // B)


def level_sse(argb, w, h, cbs, wK=0):
    orig = channels(argb, w, h)
    return {B: collage_sse(orig, B, level_wk(w, h, B, wK), q) for B, q in cbs.items()}


def leaf_table(tree, cbs, w):
    """int32 [n, 8] rows {x, y, B, idx_local, q1, q2, q3, q4} of the leaves."""
    rows = []
    for x, y, B in tree:
        j = (y // B) * (w // B) + x // B
        rows.append((x, y, B, *cbs[B][j]))
    return np.array(rows, np.int32).reshape(-1, 8)


def encode(argb, w, h, B_max, B_min, wK=0, threshold=float("inf"), cbs=None):
    cbs = cbs if cbs is not None else codebooks(argb, w, h, B_max, B_min, wK)
    sse = level_sse(argb, w, h, cbs, wK)
    return leaf_table(split(sse, w, h, B_max, B_min, threshold), cbs, w)


def write_run(leaves, w, h, B_max, B_min, wK):
    """The tag-3 stream: {3, w, h, 0, B_max, B_min, wK, n} then {B, idx_local, q1, q2, q3, q4} per leaf, big-endian."""
    hdr = np.array([3, w, h, 0, B_max, B_min, wK, len(leaves)], ">i4")
    return hdr.tobytes() + np.ascontiguousarray(np.asarray(leaves, np.int32).reshape(-1, 8)[:, 2:], ">i4").tobytes()


def read_run(run):
    """Parses and checks a tag-3 stream.  Returns (header dict, leaves int32 [n, 8]); ValueError for a malformed stream."""
    if len(run) < 32:
        raise ValueError("shorter than the header")
    tag, w, h, zero, B_max, B_min, wK, n = struct.unpack(">8i", run[:32])
    if tag != 3 or zero != 0:
        raise ValueError(f"header {tag}, {zero}")
    if B_max not in (8, 16) or B_min not in (4, 8) or B_min >= B_max:
        raise ValueError("levels")
    if w <= 0 or h <= 0 or w % B_max or h % B_max or wK < 0 or (wK == 0 and w != h):
        raise ValueError("geometry")
    wk = {B: level_wk(w, h, B, wK) for B in levels(B_max, B_min)}
    for B in wk:
        Rw, Rh, Dw, Dh = fo.geometry(w, h, B)
        if not 1 <= wk[B] <= min(Dw, Dh):
            raise ValueError("window")
    if n < 1 or n > (w // B_min) * (h // B_min) or len(run) != 32 + 24 * n:
        raise ValueError("length")
    body = np.frombuffer(run[32:], ">i4").astype(np.int32).reshape(n, 6)
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
    leaves = np.zeros((n, 8), np.int32)
    leaves[:, :3] = np.array(tree, np.int32)
    leaves[:, 3:] = body[:, 1:]
    if ((leaves[:, 3] < 0) | (leaves[:, 3] >= np.array([wk[b] ** 2 for b in leaves[:, 2]]))).any():
        raise ValueError("idx_local outside the window")
    return dict(w=w, h=h, B_max=B_max, B_min=B_min, wK=wK), leaves


def decode(run, avg_error_in=0.0):
    """The decoder loop of decodeRGB (FC:430-508) over the leaves: generateGrayImage (128 in every channel), at most 50
    iterations, each one painting every leaf from its own level's pool of scaleImageRGB of the image before the iteration;
    dR^2 + dG^2 + dB^2 per pixel in leaf order (pixel rows within a leaf) summed like Java's `avgError += (float) d`.
    Returns (rgb uint8 [H, W, 3] like fo.decode_rgb, avgError float32, iterations)."""
    hd, leaves = read_run(run)
    w, h = hd["w"], hd["h"]
    Bs = leaves[:, 2].astype(np.int64)
    offs = np.concatenate([[0], np.cumsum(Bs * Bs)[:-1]])
    per = {}
    for B in levels(hd["B_max"], hd["B_min"]):
        sel = np.nonzero(Bs == B)[0]
        if sel.size == 0:
            continue
        lv = leaves[sel]
        Rw = w // B
        j = (lv[:, 1] // B) * Rw + lv[:, 0] // B
        loc = np.zeros((h // B) * Rw, np.int32)
        loc[j] = lv[:, 3]
        gi = qm.global_index(w, h, B, level_wk(w, h, B, hd["wK"]), loc)[j]
        pos = np.arange(B * B)
        rr = lv[:, 1][:, None] + pos // B
        cc = lv[:, 0][:, None] + pos % B
        per[B] = (gi, lv[:, 3:], rr, cc, offs[sel][:, None] + pos)
    img = np.full((h, w, 3), 128, np.int64)
    avg = np.float32(avg_error_in)
    iters = 0
    for counter in range(50):
        scaled = scale_rgb(img)                                       # the pool of the image before the paint
        vals = {B: paint_values(scaled, B, gi, q) for B, (gi, q, _, _, _) in per.items()}
        sq = np.zeros(w * h, np.int64)
        for B, (_, _, rr, cc, so) in per.items():
            d = img[rr, cc] - vals[B]
            sq[so] = (d * d).sum(axis=-1)
            img[rr, cc] = vals[B]
        acc = np.add.accumulate(np.concatenate([[avg], sq.astype(np.float32)]).astype(np.float32), dtype=np.float32)
        avg = np.float32(acc[-1] / np.float32(w * h))
        iters = counter + 1
        if avg < 1:
            break
        if counter != 49:
            avg = np.float32(0.0)
    return img.astype(np.uint8), np.float32(avg), iters
