"""Reference model of the operands of the default sweep k_sweep_q (fic_q.hip) and of its prune bound.

Plain numpy, restated from the header of fic_q.hip in IEEE arithmetic (float32 / float64 / float16, round to nearest even;
numpy's float16 conversion rounds that way) with integer-exact block statistics:
  domain operand  x_i = f16(fl((d_i - dM) * w)),  w = fl(1 / (float) sqrt((double) var))          (pool_q_body)
                  folded: even f16(fl(fl((a + b - 2 dM) w) * 0.5)), odd f16(fl(fl((a - b) w) * 0.5)), b at n-1-pos
  range operand   c = copy_k - rM (folded: c + c', c - c'), exact in f16                       (k_range_q / k_range_q8)
  error bound     E_r = fl(fl(sqrtf(ss) * 7.0e-4) + 1.6e-5), ss = sum (r - rM)^2, times 2^-q_eshift (the device's sqrtf is
                  within 1 ulp of the correctly rounded root: E_r is one of three candidates, error_bound_candidates)
  acc             the exact sum of the f16 products (float64 is exact here: the products are multiples of 2^-24 below 2^17)
  q               kovarianz / sqrt(var) from the integer covariance
The MFMA's own f32 accumulation is bounded by `allowance` (header: 2^-24 * 17 NK * sum |A||B|).

Nothing here imports the HIP library: the CPU tests (tests/test_q_bound.py) run on a machine without it, and the GPU tests
(tests/test_gpu_q_bound.py) compare the device's operand bytes with these arrays bit for bit."""
import numpy as np

F32 = np.float32
ECOEF = F32(7.0e-4)
EABS = F32(1.6e-5)
LEVEL = F32(0.99999237060546875)          # 1 - 2^-17 (FIC_Q_LEVEL)
LMIN = F32(0.26)                          # FIC_Q_LMIN
TAU_ALL = F32(3.0e38)                     # FIC_Q_TAU_ALL
PAIR_FIRST = (0, 1, 4, 6)                 # folded mode: the first isometry of the pairs {0,2}, {1,3}, {4,5}, {6,7}


# ---------------------------------------------------------------------------------------------------------------------
# geometry and the grey pipeline up to the pool (make_geometry, k_scale / FC:970-1007, createCodebuch FC:1015-1050)
# ---------------------------------------------------------------------------------------------------------------------
class Geom:
    def __init__(self, w, h, B, n_iso=1):
        self.W, self.H, self.B, self.n = w, h, B, B * B
        self.lgn = int(np.log2(B * B))
        self.NK = self.n // 16
        self.Ws, self.Hs, self.abstand = w // 2, h // 2, B // 4
        self.Rw, self.Rh = w // B, h // B
        self.Nr = self.Rw * self.Rh
        self.Dw, self.Dh = 2 * self.Rw - 3, 2 * self.Rh - 3
        self.Nd = self.Dw * self.Dh
        self.n_iso = n_iso
        self.mode = 0 if n_iso == 1 else (1 if B == 4 else 2)
        self.cpr = (1, 8, 4)[self.mode]                      # sweep columns per range block


def scale(gray):
    """2:1 box average; the 4th tap is 128 where 2x + 1 >= HEIGHT (FC:993 compares a column with the height)."""
    g = np.asarray(gray, np.int64)
    H, W = g.shape
    t = g[0::2, 0::2] + g[0::2, 1::2] + g[1::2, 0::2]
    x = np.arange(W // 2)
    tap4 = np.where((2 * x + 1 >= H)[None, :], 128, g[1::2, 1::2])
    return ((t + tap4) // 4).astype(np.uint8)


def pool_pixels(gray, B):
    """[N_d, n] domain blocks of the scaled image, block d = (d % Dw, d // Dw) at (c, r) * abstand, pixel rx + ry * B."""
    G = Geom(gray.shape[1], gray.shape[0], B)
    s = scale(gray)
    out = np.zeros((G.Nd, G.n), np.uint8)
    for d in range(G.Nd):
        c, r = d % G.Dw, d // G.Dw
        out[d] = s[r * G.abstand:r * G.abstand + B, c * G.abstand:c * G.abstand + B].reshape(-1)
    return out


def range_pixels(gray, B):
    """[N_r, n] range blocks, row-major (getRangeblock FC:588-602)."""
    g = np.asarray(gray, np.uint8)
    H, W = g.shape
    return g.reshape(H // B, B, W // B, B).transpose(0, 2, 1, 3).reshape(-1, B * B)


# ---------------------------------------------------------------------------------------------------------------------
# domain operands (pool_q_body)
# ---------------------------------------------------------------------------------------------------------------------
def domain_stats(pix, B):
    """Integer statistics of DB:92-115: S, dM = S >> lgn, var = sum (d - dM)^2; s64 = sqrt((double) var); s32; w."""
    p = np.asarray(pix, np.int64)
    S = p.sum(1)
    dM = S >> int(np.log2(B * B))
    var = ((p - dM[:, None]) ** 2).sum(1)
    s64 = np.sqrt(var.astype(np.float64))
    s32 = s64.astype(F32)
    with np.errstate(divide="ignore"):
        w = np.where(var != 0, F32(1.0) / s32, F32(0.0)).astype(F32)
    return {"S": S, "dM": dM, "var": var, "s64": s64, "s32": s32, "w": w}


def domain_operands(pix, B, folded=False):
    """[N_d, n] f16 operand rows.  Plain: x at position 0..n-1.  Folded: even parts of positions 0..n/2-1, then odd parts
    (index n/2 + pos); pos is paired with n-1-pos."""
    st = domain_stats(pix, B)
    p = np.asarray(pix, np.int64)
    n = B * B
    w = st["w"][:, None]
    dM = st["dM"][:, None]
    if not folded:
        return ((p - dM).astype(F32) * w).astype(np.float16)
    a, b = p[:, :n // 2], p[:, ::-1][:, :n // 2]
    even = (((a + b - 2 * dM).astype(F32) * w) * F32(0.5)).astype(np.float16)
    odd = (((a - b).astype(F32) * w) * F32(0.5)).astype(np.float16)
    return np.concatenate([even, odd], 1)


def dflat(pix, B, Nd, ntiles):
    """1 for a domain tile (32 blocks) whose blocks are all flat or beyond N_d."""
    st = domain_stats(pix, B)
    nonflat = np.zeros(ntiles * 32, bool)
    nonflat[:Nd] = st["var"][:Nd] != 0
    return (~nonflat.reshape(ntiles, 32).any(1)).astype(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# range operands (k_range_q, k_range_q8, k_prep_q8)
# ---------------------------------------------------------------------------------------------------------------------
def iso_source(k, B, x, y):
    """fic_devfn.h iso_source (shared with the oracle's fo_iso_source): out[y][x] = d[sy][sx]."""
    m = B - 1
    sx, sy = {0: (x, y), 1: (y, m - x), 2: (m - x, m - y), 3: (m - y, x),
              4: (m - x, y), 5: (x, m - y), 6: (y, x), 7: (m - y, m - x)}[k]
    return sx + sy * B


def iso_inverse(k):
    return 3 if k == 1 else (1 if k == 3 else k)


def iso_copy_index(k, B):
    """copy_k[pos] = r[idx[pos]] so that dot(copy_k, d) == dot(r, iso_k(d))."""
    ki = iso_inverse(k)
    return np.array([iso_source(ki, B, p % B, p // B) for p in range(B * B)])


def range_stats(rpix, B, eshift=0):
    """rM, rem = S - n rM (varianzRange), ss = sum (r - rM)^2 and E_r as the range-prep kernels store it."""
    r = np.asarray(rpix, np.int64)
    n = B * B
    S = r.sum(1)
    rM = S >> int(np.log2(n))
    rem = S - rM * n
    ss = ((r - rM[:, None]) ** 2).sum(1)
    E = error_bound(ss, eshift)
    return {"S": S, "rM": rM, "rem": rem, "ss": ss, "E": E, "E_lo": error_bound(ss, eshift, -1)}


def error_bound(ss, eshift=0, sqrt_ulps=0):
    """E_r from ss.  The kernels' __fsqrt_rn is the hardware square root here (v_sqrt_f32, within 1 ulp of the correctly
    rounded one, not always equal to it): sqrt_ulps = -1 / +1 gives the neighbours of the correctly rounded root, and
    error_bound_candidates all three (the device's E_r is one of them; the bound checks use the smallest)."""
    r = np.sqrt(np.asarray(ss).astype(F32)).astype(F32)
    if sqrt_ulps:
        r = np.where(r > 0, np.nextafter(r, F32(np.inf) if sqrt_ulps > 0 else F32(0)), r).astype(F32)
    E = (r * ECOEF) + EABS
    return (E.astype(F32) * F32(2.0 ** -eshift)).astype(F32)


def error_bound_candidates(ss, eshift=0):
    return np.stack([error_bound(ss, eshift, u) for u in (-1, 0, 1)])


def range_columns(rpix, B, n_iso):
    """[N_r * cpr, n] integer operand columns: mode 0 c = r - rM; mode 1 the 8 copies c_k (column 8 j + k); mode 2 per
    isometry pair (column 4 j + c, first isometry PAIR_FIRST[c]) the even part c + c' of positions 0..n/2-1, then the odd
    part c - c' (c' at n-1-pos, the pair's partner)."""
    r = np.asarray(rpix, np.int64)
    n = B * B
    rM = r.sum(1) >> int(np.log2(n))
    mode = 0 if n_iso == 1 else (1 if B == 4 else 2)
    if mode == 0:
        return r - rM[:, None]
    ks = range(8) if mode == 1 else PAIR_FIRST
    cols = []
    for k in ks:
        c = r[:, iso_copy_index(k, B)] - rM[:, None]
        if mode == 2:
            c = np.concatenate([c[:, :n // 2] + c[:, ::-1][:, :n // 2], c[:, :n // 2] - c[:, ::-1][:, :n // 2]], 1)
        cols.append(c)
    return np.stack(cols, 1).reshape(-1, n)


def copies(rpix, B):
    """[N_r, 8, n] the isometry copies as bytes (rngC of mode 1)."""
    r = np.asarray(rpix)
    return np.stack([r[:, iso_copy_index(k, B)] for k in range(8)], 1)


# ---------------------------------------------------------------------------------------------------------------------
# device fragment layouts -> [plane][row][element]
# ---------------------------------------------------------------------------------------------------------------------
def frag_map(NK, shape16):
    """(row, element) of every (slot m, lane, u) of a 32-row fragment tile (frag_slot in fic_q.hip): arrays [NK, 64, 8]."""
    m = np.arange(NK)[:, None, None]
    lane = np.arange(64)[None, :, None]
    u = np.arange(8)[None, None, :]
    if not shape16:
        row = np.broadcast_to(lane & 31, (NK, 64, 8))
        el = 16 * m + 8 * (lane >> 5) + u
    else:
        KS = NK // 2
        row = 16 * (m // KS) + (lane & 15)
        el = 32 * (m % KS) + 8 * (lane >> 4) + u
    return np.broadcast_to(row, (NK, 64, 8)), np.broadcast_to(el, (NK, 64, 8))


def decode_frags(raw, n, shape16=0):
    """Fragment store [..., tiles, NK, 64] of 8 f16 each (raw uint8 / float16 buffer) -> [..., tiles * 32, n] float16.
    The folded layout needs no other map: slot m < NK/2 holds even parts [16m + 8h, +8), slot m >= NK/2 odd parts
    [16(m - NK/2) + 8h, +8) = operand index 16m + 8h - n/2 + n/2."""
    NK = n // 16
    f = np.asarray(raw).view(np.float16)
    lead = f.shape[:-1]
    f = f.reshape(lead + (-1, NK, 64, 8))
    tiles = f.shape[-4]
    row, el = frag_map(NK, shape16)
    out = np.zeros(lead + (tiles, 32, n), np.float16)
    out[..., row, el] = f
    return out.reshape(lead + (tiles * 32, n))


# ---------------------------------------------------------------------------------------------------------------------
# the prune test's values and the exact reference values
# ---------------------------------------------------------------------------------------------------------------------
def acc_exact(A, Bc):
    """[rows of A, rows of Bc] exact sums of the f16 products (float64: the products are multiples of 2^-24 below 2^10 *
    2^9 and their sums stay below 2^29 * 2^24)."""
    return np.asarray(A, np.float64) @ np.asarray(Bc, np.float64).T


def allowance(A, Bc, NK):
    """Accumulation error of the f32 MFMA chain, header of fic_q.hip: 2^-24 * 17 NK * sum |A||B|."""
    return 2.0 ** -24 * 17 * NK * (np.abs(np.asarray(A, np.float64)) @ np.abs(np.asarray(Bc, np.float64)).T)


def q_exact(pix, rcols_int, B, folded=False):
    """Real-valued counterpart of acc_exact from the integer covariance: sum c_i (d_i - dM) / sqrt(var) (folded: the even
    and odd parts Be = sum (c + c')(x + x')/2, Bo = sum (c - c')(x - x')/2 with x = (d - dM) / sqrt(var)).  float64 of an
    exact integer over a correctly rounded square root."""
    st = domain_stats(pix, B)
    p = np.asarray(pix, np.int64) - st["dM"][:, None]
    n = B * B
    if folded:
        a, b = p[:, :n // 2], p[:, ::-1][:, :n // 2]
        p = np.concatenate([a + b, a - b], 1)                # 2 x the even / odd parts of d - dM
    cov = p @ np.asarray(rcols_int, np.int64).T
    with np.errstate(divide="ignore", invalid="ignore"):
        q = cov / st["s64"][:, None]
    q[st["var"] == 0] = 0.0
    return q / 2.0 if folded else q


def parts(A, Bc, folded):
    """acc (plain) or (acc_even, acc_odd) (folded), each [rows of A, rows of Bc], exact."""
    if not folded:
        return (acc_exact(A, Bc),)
    h = np.asarray(A).shape[1] // 2
    return acc_exact(np.asarray(A)[:, :h], np.asarray(Bc)[:, :h]), acc_exact(np.asarray(A)[:, h:], np.asarray(Bc)[:, h:])


def prune_value(A, Bc, folded):
    """The epilogue's value per (domain block, column) from the exact sums: |acc| or, folded, |even| + |odd| -- the larger
    |q| of the isometry pair.  (The device adds MFMA rounding, within `allowance`, and rounds the folded sum to f32.)"""
    p = parts(A, Bc, folded)
    return np.abs(p[0]) if not folded else np.abs(p[0]) + np.abs(p[1])


def exact_error(cov, rem, s64):
    """fic_devfn.h exact_error / getErrorVarianceCovariance FC:674-683 (numpy, elementwise)."""
    cov = np.asarray(cov, np.float64)
    remf = np.asarray(rem).astype(F32)
    s64 = np.asarray(s64, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where((np.asarray(rem) == 0) | (s64 == 0.0), F32(0.0),
                     (cov / (remf.astype(np.float64) * s64)).astype(F32)).astype(F32)
    r = r * r
    return ((remf * remf) * (F32(1.0) - r)).astype(F32)


def theta_from_pair(m, E):
    """theta after evaluating a pair with test value m: fl(fl((m - E) * (1 - 2^-17)) - E) (both updates of slow_tile)."""
    m, E = F32(m), F32(E)
    return F32(F32(F32(m - E) * LEVEL) - E)


# ---------------------------------------------------------------------------------------------------------------------
# inputs that push pairs against the bound
# ---------------------------------------------------------------------------------------------------------------------
# (B, n_iso) -> image side, share of the rows that hold domain probes
TIGHT_SHAPES = {(4, 1): (128, 0.5), (4, 8): (128, 0.5), (8, 1): (256, 0.5), (8, 8): (256, 0.5), (16, 1): (512, 0.75),
                (16, 8): (384, 0.75)}


def tight_image(B, n_iso, seed=1, bg=40, band=0.12, size=None):
    """A grey image whose range blocks sit against the prune bound.  Top rows: "domain probes" -- pairs of horizontally
    adjacent spikes in the SCALED image (every scaled pixel made from a uniform 2x2 cell), one pair per (B + 2) x B cell, so
    that a domain block holds at most one pair; heights h1, h2 = h1 * (1 +- band).  Bottom rows: "range probes" -- every
    range block a pair of spikes a1, a2 = a1 * (1 +- band) at positions (1, 1), (2, 1).  A range block is matched by the
    domain blocks whose pair sits at the same position, all of nearly the same direction (h1 : h2 close to a1 : a2): their
    exact q differ by little, while the f16 roundings of their two or three distinct normalised values differ by a sizeable
    share of E_r, either way.  So many ranges have a pair X in an earlier domain tile with |acc_X| well above |acc_W| of the
    exact winner W -- what a too-small E_r turns into a pruned winner (prune_witnesses counts them).  `size` overrides the
    image side (a larger pool, e.g. for long pool chunks)."""
    S, frac = TIGHT_SHAPES[(B, n_iso)]
    S = S if size is None else size
    rng = np.random.default_rng(seed)
    g = np.full((S, S), bg, np.int64)
    top = int(S * frac) // (2 * B) * (2 * B)
    sc = np.full((top // 2, S // 2), bg, np.int64)
    for y in range(1, top // 2 - 1, B):
        for x in range(1, S // 2 - 2, B + 2):
            h1 = int(rng.integers(120, 210))
            sc[y, x], sc[y, x + 1] = bg + h1, bg + int(h1 * rng.uniform(1 - band, 1 + band))
    g[:top] = np.repeat(np.repeat(sc, 2, 0), 2, 1)
    for by in range(top // B, S // B):
        for bx in range(S // B):
            a1 = int(rng.integers(120, 210))
            g[by * B + 1, bx * B + 1], g[by * B + 1, bx * B + 2] = bg + a1, bg + int(a1 * rng.uniform(1 - band, 1 + band))
    return np.clip(g, 0, 255).astype(np.uint8), (top // B) * (S // B)


def pair_column(iso, mode):
    """Sweep column (within the range block) that tests isometry `iso`."""
    if mode == 0:
        return 0
    if mode == 1:
        return iso
    return PAIR_FIRST.index({0: 0, 2: 0, 1: 1, 3: 1, 4: 4, 5: 4, 6: 6, 7: 6}[int(iso)])


def sweep_tables(gray, B, n_iso, eshift=0):
    """Everything the prune test of one grey plane sees, from the model: operands, test values (exact sums), the
    accumulation allowance, range statistics."""
    H, W = gray.shape
    G = Geom(W, H, B, n_iso)
    folded = G.mode == 2
    pix = pool_pixels(gray, B)
    A = domain_operands(pix, B, folded)
    rp = range_pixels(gray, B)
    rs = range_stats(rp, B, eshift)
    cols = range_columns(rp, B, n_iso)
    val = prune_value(A, cols.astype(np.float16), folded)
    allow = allowance(A, cols.astype(np.float16), G.NK)
    return {"G": G, "pix": pix, "A": A, "cols": cols, "rs": rs, "val": val, "allow": allow, "folded": folded}


def prune_witnesses(T, winners, isos, s, r0=0):
    """Per range block j >= r0 (rem != 0): does a pair X of a domain tile BEFORE the exact winner's tile reach a theta, with
    E_r shrunk to s E_r, above the winner's test value?  Then a one-chunk sweep with that E_r skips the winner.  Returns a
    bool array over ranges r0.. and the largest (|acc_X| - |acc_W|) / E_r per range (the inputs' tightness)."""
    G, val, allow, rs = T["G"], T["val"], T["allow"], T["rs"]
    hit = np.zeros(G.Nr - r0, bool)
    tight = np.zeros(G.Nr - r0)
    for j in range(r0, G.Nr):
        if rs["rem"][j] == 0:
            continue
        E = float(rs["E"][j])
        w, c = int(winners[j]), j * G.cpr + pair_column(isos[j], G.mode)
        vW = val[w, c] + allow[w, c]
        t = (w // 32) * 32
        if t == 0:
            continue
        blk = slice(j * G.cpr, (j + 1) * G.cpr)
        vX = (val[:t, blk] - allow[:t, blk]).max()
        tight[j - r0] = (vX - vW) / E
        hit[j - r0] = float(theta_from_pair(vX, F32(s * E))) >= vW
    return hit, tight


# ---------------------------------------------------------------------------------------------------------------------
# joint RGB (k_scale_rgb, k_pool_rgb, k_range_rgb -> k_pool_qrgb, k_range_qrgb)
# ---------------------------------------------------------------------------------------------------------------------
def scale_rgb(rgb):
    """k_scale_rgb per channel: (p00 + p10 + p01 + p01) / 4 -- the reference's 4th tap repeats the lower-left pixel, or is
    128 where 2x + 1 >= HEIGHT."""
    c = np.asarray(rgb, np.int64)
    H, W = c.shape[:2]
    p00, p10, p01 = c[0::2, 0::2], c[0::2, 1::2], c[1::2, 0::2]
    x = np.arange(W // 2)
    tap4 = np.where((2 * x + 1 >= H)[None, :, None], 128, p01)
    return ((p00 + p10 + p01 + tap4) // 4).astype(np.int64)


def rgb_pool(rgb, B):
    """pool_sum [N_d, n] (R + G + B per pool pixel), msum (sum of the channel means), vD = sum greyD_i (exact)."""
    G = Geom(rgb.shape[1], rgb.shape[0], B)
    s = scale_rgb(rgb)
    blk = np.zeros((G.Nd, G.n, 3), np.int64)
    for d in range(G.Nd):
        c, r = d % G.Dw, d // G.Dw
        blk[d] = s[r * G.abstand:r * G.abstand + B, c * G.abstand:c * G.abstand + B].reshape(-1, 3)
    msum = (blk.sum(1) >> G.lgn).sum(1)
    psum = blk.sum(2)
    return psum, msum, psum.sum(1) - G.n * msum


def rgb_range(rgb, B):
    """greyR [N_r, n] = R + G + B - msum per pixel, vR = sum greyR_i (varianzRange)."""
    c = np.asarray(rgb, np.int64)
    H, W = c.shape[:2]
    blk = c.reshape(H // B, B, W // B, B, 3).transpose(0, 2, 1, 3, 4).reshape(-1, B * B, 3)
    msum = (blk.sum(1) >> int(np.log2(B * B))).sum(1)
    g = blk.sum(2) - msum[:, None]
    return g, g.sum(1)


def _sqrt_f32(x, ulps=0):
    r = np.sqrt(np.asarray(x).astype(F32)).astype(F32)
    if ulps:
        r = np.where(r > 0, np.nextafter(r, F32(np.inf) if ulps > 0 else F32(0)), r).astype(F32)
    return r


def rgb_domain_operands(psum, msum, vD, sqrt_ulps=0):
    """A [N_d, n] = f16(fl(greyD_i / vD)) (zero rows for vD == 0) and the rounded-up norms fl(fl(sqrtf(s2) / vD) * 1.001)
    whose maximum is Amax (k_pool_qrgb; sqrt_ulps as in error_bound)."""
    gd = np.asarray(psum, np.int64) - np.asarray(msum, np.int64)[:, None]
    vd = np.asarray(vD).astype(F32)[:, None]
    live = np.asarray(vD) != 0
    with np.errstate(divide="ignore", invalid="ignore"):
        A = np.where(live[:, None], gd.astype(F32) / vd, F32(0)).astype(np.float16)
        s2 = (gd * gd).sum(1)
        norm = ((_sqrt_f32(s2, sqrt_ulps) / vd[:, 0]).astype(F32) * F32(1.001)).astype(F32)
    return A, np.where(live, norm, F32(0)).astype(F32)


def rgb_error_bound(greyR, amax, eshift=0, sqrt_ulps=0):
    """k_range_qrgb: fl(fl(fl(fl(sqrtf(s2) * 1.0001) * Amax) * 7.0e-4) + fl(1.6e-5 * fl(1 + Amax))) * 2^-q_eshift."""
    s2 = (np.asarray(greyR, np.int64) ** 2).sum(1)
    am = F32(amax)
    E = (((_sqrt_f32(s2, sqrt_ulps) * F32(1.0001)).astype(F32) * am).astype(F32) * ECOEF).astype(F32) + F32(EABS * F32(F32(1) + am))
    return (E.astype(F32) * F32(2.0 ** -eshift)).astype(F32)


def rgb_kov_java(greyR, psum, msum):
    """kovarianz as the reference accumulates it: f32, i = 0..n-1, [N_d, N_r] (FC:781-791)."""
    gd = (np.asarray(psum, np.int64) - np.asarray(msum, np.int64)[:, None]).astype(np.int64)
    gr = np.asarray(greyR, np.int64)
    kov = np.zeros((gd.shape[0], gr.shape[0]), F32)
    for i in range(gd.shape[1]):
        kov = (kov + np.outer(gd[:, i], gr[:, i]).astype(F32)).astype(F32)
    return kov


# ---------------------------------------------------------------------------------------------------------------------
# colour inputs that push pairs against the joint-RGB bound
# ---------------------------------------------------------------------------------------------------------------------
# B -> image side, share of the rows that hold domain probes, h1_c + h2_c of every probe pair per channel (= rho_c mod n)
# (chosen among a few sums per block size for the roundings of greyD / vD: vD = 5 / 3 / 13)
TIGHT_RGB_SHAPES = {4: (128, 0.5, (226, 226, 225)), 8: (256, 0.5, (257, 257, 257)), 16: (512, 0.75, (261, 260, 260))}


# The smallest q_eshift (E_r times 2^-q_eshift) at which the model finds prune witnesses on the committed generator, seed 1
# (tests/test_q_bound.py asserts it; tests/test_gpu_rgb_q_bound.py shrinks the device's E_r by it).  1 is undetectable.
TIGHT_RGB_ESHIFT = {4: 2, 8: 2, 16: 2}


def tight_rgb_image(B, seed=1, size=None, bg=40, band=0.12):
    """A colour image whose range blocks sit against the joint-RGB prune bound, and the first probe range r0.

    q = kovarianz / vD is not normalised by the domain block's norm, and E_r carries the pool-wide factor Amax = max ||greyD|| /
    vD: the bound is tight only where the competing blocks have ||greyD|| / vD close to Amax, so the generator fixes vD and
    the norm of EVERY non-flat block of the pool.
      * Top rows, "domain probes": spike pairs (h1, h2 per channel) at x, x + 2 of one row of the SCALED image (uniform 2x2
        cells), one pair per (pitch x B) cell, pitch = B + 2 rounded up to a multiple of abstand: a domain block holds a whole
        pair, one spike of a cut pair, or nothing.  Per channel h1_c + h2_c is the same constant for all pairs, = rho_c mod
        n: every block with a whole pair has vD = sum rho_c (5, 3, 13: greyD / vD rounds in f16), the same floor term, and
        ||greyD|| within 1 % (H1 + H2 constant, H1 : H2 within 1 +- band) -- these blocks are Amax.  A block with one spike has
        vD = sum (h_c mod n) >= 6 by construction (residues 0 and 1 are rejected) and at most half the squared norm; all other
        blocks are flat (vD = 0).
      * Bottom rows, "range probes": spikes a1, a2 = a1 - (0..2 per channel) at (1, 1) and (3, 1) of every range block -- odd
        coordinates, which the reference's colour down-scaling never reads (its 4th tap repeats the lower-left pixel), so
        the pool under the range probes is flat and cannot set Amax.
    With H1 + H2 constant, q of the matching blocks is const + (A1 - A2) H1 / vD: all of them lie within a fraction of E_r of
    each other, while the f16 roundings of (H1 - eps) / vD and (H2 - eps) / vD differ by a sizeable share of E_r.  The pair with
    the largest H1 and the one with the smallest come last in the pool, so the exact winner of every probe range has the
    other candidates in earlier domain tiles (rgb_prune_witnesses)."""
    S, frac, csum = TIGHT_RGB_SHAPES[B]
    S = S if size is None else size
    n, ab = B * B, B // 4
    pitch = -(-(B + 2) // ab) * ab
    rng = np.random.default_rng(seed)
    top = int(S * frac) // (2 * B) * (2 * B)
    sc = np.full((top // 2, S // 2, 3), bg, np.int64)
    cells = [(x, y) for y in range(1, top // 2 - 1, B) for x in range(1, S // 2 - 3, pitch)]
    pairs = []
    while len(pairs) < len(cells):
        h1 = np.array([int(round(c / 2 * rng.uniform(1 - band, 1 + band))) for c in csum])
        h2 = np.array(csum) - h1
        if all(1 <= h <= 255 - bg and h % n >= 2 for h in list(h1) + list(h2)):
            pairs.append((h1, h2))
    # The pair with the largest H1 and the one with the smallest come last in the pool (the exact winners of the probe ranges
    # with A1 > A2 and A1 < A2), each moved 1..7 further out to the step whose two f16 roundings fall lowest: the winner's
    # test value then lies below its q, the near-equal candidates of the earlier tiles above theirs.
    eps, vd = sum(c // n for c in csum), sum(c % n for c in csum)

    def low(h1):
        x = np.array([h1.sum() - eps, sum(csum) - h1.sum() - eps], np.int64)
        return float(((x.astype(F32) / F32(vd)).astype(np.float16).astype(np.float64) - x / vd).sum())

    def ok(h1):
        return all(1 <= h <= 255 - bg and h % n >= 2 for h in list(h1) + list(np.array(csum) - h1))

    H1 = [int(p[0].sum()) for p in pairs]
    ends = []
    for i, sgn in ((int(np.argmin(H1)), -1), (int(np.argmax(H1)), 1)):
        cand = []
        for k in range(1, 8):
            for c in range(3):
                h1 = pairs[i][0] + sgn * np.array([k // 3 + (1 if (j - c) % 3 < k % 3 else 0) for j in range(3)])
                if ok(h1):
                    cand.append((low(h1), k, c, h1))
        h1 = min(cand, key=lambda t: t[:3])[3]
        ends.append((h1, np.array(csum) - h1))
    keep = [p for i, p in enumerate(pairs) if i not in (int(np.argmin(H1)), int(np.argmax(H1)))]
    pairs = keep + ends
    order = range(len(pairs))
    for (x, y), i in zip(cells, order):
        sc[y, x], sc[y, x + 2] = bg + pairs[i][0], bg + pairs[i][1]
    g = np.full((S, S, 3), bg, np.int64)
    g[:top] = np.repeat(np.repeat(sc, 2, 0), 2, 1)
    for by in range(top // B, S // B):
        for bx in range(S // B):
            a1 = rng.integers(150, 211, 3)
            d = rng.integers(0, 3, 3)
            if d.sum() == 0:
                d[int(rng.integers(0, 3))] = 1
            sgn = 1 if rng.integers(0, 2) else -1
            g[by * B + 1, bx * B + 1], g[by * B + 1, bx * B + 3] = bg + a1, bg + a1 - sgn * d
    return np.clip(g, 0, 255).astype(np.uint8), (top // B) * (S // B)


def rgb_sweep_tables(rgb, B, eshift=0):
    """Everything the prune test of one colour image sees, from the model (the colour analogue of sweep_tables): operands,
    test values |acc| (exact sums of the f16 products), the accumulation allowance, vR, and E_r with the square roots one ulp
    low (the smallest E_r the device can store)."""
    H, W = rgb.shape[:2]
    G = Geom(W, H, B)
    psum, msum, vD = rgb_pool(rgb, B)
    gR, vR = rgb_range(rgb, B)
    A, norm = rgb_domain_operands(psum, msum, vD, -1)
    amax = norm.max()
    E = rgb_error_bound(gR, amax, eshift, -1)
    Bc = gR.astype(np.float16)
    return {"G": G, "psum": psum, "msum": msum, "vD": vD, "gR": gR, "A": A, "norm": norm, "amax": amax,
            "rs": {"rem": vR, "E": E}, "val": np.abs(acc_exact(A, Bc)), "allow": allowance(A, Bc, G.NK), "folded": False}


def rgb_prune_witnesses(T, winners, s, r0=0):
    """prune_witnesses for the tables of rgb_sweep_tables; `winners` are the oracle's (encode_rgb, full search)."""
    return prune_witnesses(T, winners, np.zeros(len(winners), np.int64), s, r0)
