"""numpy restatement of the matrix-core joint-RGB least-squares sweep (fic_lsq_rgb_q.hip): the operands
and the per-range constants of k_lsq_rgb_q_prep in IEEE float32 / float16 (round to nearest even, subnormals kept, as numpy
converts; `flushed` gives the other matrix unit), the float chain of theta, and the sweep itself -- tile by tile, theta raised
only after a tile's flagged pairs are evaluated, every tile in 16 rounds with the second stage's tau refined between them, as
the kernel does at all three block sizes.  It follows tests/lsqqmodel.py.  Test infrastructure only; nothing here touches a GPU.

A block is one vector of K = 3 n entries, element i = ch * n + pos.
  A row     x_i = f16(fl((float)(n d_i - S_d[ch]) * w)),  w = fl(1 / fl(B * s32)),  s32 = fl32(sqrt((double) V));  V == 0: zeros
  B column  copy_k[i] - m_r[ch],  m_r[ch] = floor((2 S_r[ch] + n) / (2 n));  column j * n_iso + k
  R         n S_rr - sum_ch S_r[ch]^2
  Er        fl(fl(fl(sqrt(ss)) * c) + 1.6e-5) * 2^-eshift,  ss = sum (r_i - m_r[ch])^2,
            c = fl(fl(7.0e-4f + fl(NK * 1.1e-6f)) + fl(B * 1.0575e-4f)),  NK = 3 n / 16
  theta     fl(tau * (1 / B) - Er),  tau = fl(fl(fl(sqrtf(fl(Ti)) * 0.001f) * (1 - 2^-18)) * widen),  Ti = 10^6 R - n E_best;
            a negative difference times 1 + 2^-22.  A flagged pair is evaluated only if |C| > li = trunc(fl(tau * s32)), the test
            of k_sweep_lsq_rgb_fast (lsqtight.li_model(rgb=True)), in 64 bits at B = 16
The two float roots are correctly rounded on paper; the hardware's are within 1 ulp, so `ulps` = -1 / +1 gives the neighbours."""
import numpy as np

import lsqtight as lt
import qmodel
import qtmodel

F32 = np.float32
I64 = np.int64
ECOEF = F32(7.0e-4)
EACC = F32(1.1e-6)
ESUB = F32(1.0575e-4)
EABS = F32(1.6e-5)
SAFETY = F32(0.99999618530273437500)      # 1 - 2^-18 (FIC_LSQ_TAU_SAFETY)
NEVER = F32(3.0e38)                       # theta "never flagged"
CTW = {4: 4, 8: 2, 16: 1}                 # column tiles a wave keeps (lsq_rgb_q_ctw)
SCALE = 10 ** 6                           # E is this many times the squared error


def kernel_name(B, n_iso):
    return f"k_sweep_lsq_rgb_q<{3 * B * B // 16}, {3 if n_iso == 8 else 0}>"


def planar(blocks):
    """[N, n, 3] (the models' order) -> int64 [N, 3 n], element ch * n + pos (the stores' order)."""
    b = np.asarray(blocks, I64)
    return b.transpose(0, 2, 1).reshape(b.shape[0], -1)


# ---------------------------------------------------------------------------------------------------------------------
# the prep
# ---------------------------------------------------------------------------------------------------------------------
def pool_stats(pool):
    """S_d [N_d, 3], S_dd, V (int64 [N_d]) and s32 of pool blocks [N_d, n, 3]."""
    p = np.asarray(pool, I64)
    n = p.shape[1]
    S, Q = p.sum(1), (p * p).sum((1, 2))
    V = n * Q - (S * S).sum(1)
    return S, Q, V, np.sqrt(V.astype(np.float64)).astype(F32)


def a_rows(pool, B):
    """float16 [N_d, 3 n]: the A operand rows."""
    p = np.asarray(pool, I64)
    n = B * B
    S, _, V, s32 = pool_stats(p)
    with np.errstate(divide="ignore"):
        w = np.where(V != 0, F32(1.0) / (F32(B) * s32), F32(0.0)).astype(F32)
    x = planar(n * p - S[:, None, :]).astype(F32) * w[:, None]
    assert x.dtype == F32
    return x.astype(np.float16)


def flushed(A):
    """The A rows as a matrix unit that flushed f16 subnormals would see them."""
    A = np.asarray(A, np.float16)
    return np.where(np.abs(A.astype(np.float64)) < 2.0 ** -14, np.float16(0), A)


def copies(rblocks, B, n_iso):
    """int64 [N_r, n_iso, n, 3]: copy_k with sum_p copy_k[p] d[p] = sum_i r[i] d[iso_k[i]] (the copies of rng3)."""
    r = np.asarray(rblocks, I64)
    iso = qtmodel.iso_table(B)[:n_iso]
    out = np.empty((r.shape[0], n_iso) + r.shape[1:], I64)
    for k in range(n_iso):
        out[:, k, iso[k]] = r
    return out


def root32(x, ulps=0):
    r = np.sqrt(np.asarray(x).astype(F32)).astype(F32)
    if ulps:
        r = np.where(r > 0, np.nextafter(r, F32(np.inf) if ulps > 0 else F32(0)), r).astype(F32)
    return r


def ecoef(B):
    NK = 3 * B * B // 16
    return F32(F32(ECOEF + F32(NK) * EACC) + F32(B) * ESUB)


def allowance_er(ss, B, eshift=0, ulps=0):
    e = (root32(ss, ulps) * ecoef(B)) + EABS
    assert e.dtype == F32
    return (e * F32(2.0 ** -eshift)).astype(F32)


def range_stats(rblocks, B, eshift=0):
    """dict of per-range arrays: S_r, m_r [N_r, 3], S_rr, ss, R (int64 [N_r]), Er (float32, correctly rounded root) and Er3
    [3, N_r] (root -1 / 0 / +1 ulp)."""
    r = np.asarray(rblocks, I64)
    n = B * B
    lgn = int(np.log2(n))
    S, Q = r.sum(1), (r * r).sum((1, 2))
    mr = (2 * S + n) >> (lgn + 1)
    ss = Q - 2 * (mr * S).sum(1) + n * (mr * mr).sum(1)
    assert (ss == ((r - mr[:, None, :]) ** 2).sum((1, 2))).all() and (ss < 2 ** 24).all()
    R = n * Q - (S * S).sum(1)
    assert (R >= 0).all() and (R < 2 ** 32).all()
    return {"S_r": S, "S_rr": Q, "m_r": mr, "ss": ss, "R": R, "Er": allowance_er(ss, B, eshift),
            "Er3": np.stack([allowance_er(ss, B, eshift, u) for u in (-1, 0, 1)])}


def b_columns(rblocks, B, n_iso):
    """int64 [N_r * n_iso, 3 n]: the B operand columns (exact in f16)."""
    st = range_stats(rblocks, B)
    c = copies(rblocks, B, n_iso) - st["m_r"][:, None, None, :]
    return planar(c.reshape((-1,) + c.shape[2:]))


def decode_frags(raw, n3, rows):
    """Device fragment store (raw bytes, one plane or several) -> float16 [..., rows, 3 n] (the 32x32x16 layout of frag_slot)."""
    return qmodel.decode_frags(raw, n3)[..., :rows, :]


def q_exact(pool, cols, B):
    """float64 [N_d, columns]: C / sqrt(n V) from the exact integer C = sum (n d_i - S_d[ch]) b_i (0 where V == 0)."""
    p = np.asarray(pool, I64)
    n = B * B
    S, _, V, _ = pool_stats(p)
    C = planar(n * p - S[:, None, :]) @ np.asarray(cols, I64).T
    with np.errstate(divide="ignore", invalid="ignore"):
        q = C / np.sqrt((n * V).astype(np.float64))[:, None]
    q[V == 0] = 0.0
    return q


# ---------------------------------------------------------------------------------------------------------------------
# theta
# ---------------------------------------------------------------------------------------------------------------------
def theta(Ti, Er, B, widen=0, ulps=0, safety=SAFETY):
    """theta of the kernel for Ti = 10^6 T >= 0 (int64) and the range's Er, elementwise, float32."""
    Ti = np.asarray(Ti, I64)
    assert (Ti >= 0).all()
    tau = (root32(Ti, ulps) * F32(0.001)) * F32(safety)
    tau = tau * F32(1.0 + 2.0 ** -widen if widen else 1.0)
    assert tau.dtype == F32
    th = (tau * F32(1.0 / B) - np.asarray(Er, F32)).astype(F32)
    return np.where(th < 0, th * F32(1.0 + 2.0 ** -22), th).astype(F32)


def theta_update(R, E_best, Er, B, widen=0):
    """theta after the range's smallest evaluated E became E_best: "never flagged" on an exact hit, -1 where T < 0."""
    R, E_best = np.asarray(R, I64), np.asarray(E_best, I64)
    Ti = SCALE * R - B * B * E_best
    th = theta(np.maximum(Ti, 0), Er, B, widen)
    th = np.where(Ti < 0, F32(-1.0), th)
    return np.where(E_best == 0, NEVER, th).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------
# the sweep
# ---------------------------------------------------------------------------------------------------------------------
ROUNDS = [[(e & 3) + 8 * (e >> 2), (e & 3) + 8 * (e >> 2) + 4] for e in range(16)]
_SUMS = {}                                # the exact sums of the last few images (a test sweeps one image under several settings)


def _pair_sums(rgb, B, n_iso):
    key = (rgb.shape, B, n_iso, rgb.tobytes())
    if key not in _SUMS:
        if len(_SUMS) >= 4:
            _SUMS.pop(next(iter(_SUMS)))
        _SUMS[key] = lt.pair_sums(rgb, B, n_iso, True)
    return _SUMS[key]


def sweep(rgb, B, n_iso, eshift=0, widen=0, tiles_per_chunk=None, bias=0.0, flush=False):
    """The sweep of k_sweep_lsq_rgb_q on one image uint8 [H, W, 3], full search: dict with E, c (int64 [N_r]), idx_local, iso,
    exact (pairs the GEMM flagged) and pairs.  acc is the exact sum of the f16 products (the device's f32 accumulation differs
    within qmodel.allowance; `bias` times that allowance is added to |acc| before the test, for a derivation that wants to be on
    one side of it).  flush: the A operand with f16 subnormals flushed."""
    rgb = np.ascontiguousarray(rgb, np.uint8)
    n = B * B
    NK = 3 * n // 16
    pool = lt._pool(rgb, B, True)                                            # [N_d, n, 3]
    r = lt._blocks(rgb, B)                                                   # [N_r, n, 3]
    nr, nd = r.shape[0], pool.shape[0]
    s = _pair_sums(rgb, B, n_iso)
    E, C, V = s["E"], np.abs(s["C"]), s["V"]                                 # [N_r, N_d, n_iso], [N_d]
    st = range_stats(r, B, eshift)
    assert (st["R"] == s["R"]).all()
    A, Bc = a_rows(pool, B), b_columns(r, B, n_iso)
    if flush:
        A = flushed(A)
    acc = np.abs(qmodel.acc_exact(A, Bc))
    if bias:
        acc = acc + bias * qmodel.allowance(A, Bc, NK)
    acc = acc.reshape(nd, nr, n_iso).transpose(1, 0, 2)                      # [N_r, N_d, n_iso]
    ndt = (nd + 31) // 32
    tpc = ndt if tiles_per_chunk is None else tiles_per_chunk
    BIG = np.iinfo(I64).max
    best_E, best_c, exact = np.full(nr, BIG), np.full(nr, BIG), 0
    cidx = (np.arange(nd)[:, None] * n_iso + np.arange(n_iso)[None, :])[None]
    for t0 in range(0, ndt, tpc):
        th = np.full(nr, F32(-1.0))
        Ti = np.full(nr, -1, I64)                                             # 10^6 T behind theta; < 0: no second-stage skip
        cE, cc = np.full(nr, BIG), np.full(nr, BIG)
        for t in range(t0, min(t0 + tpc, ndt)):
            sl = slice(32 * t, min(32 * t + 32, nd))
            flag = ~(acc[:, sl] <= th[:, None, None].astype(np.float64))
            exact += int(flag.sum())
            # 16 rounds, rows (e & 3) + 8 (e >> 2) and 4 more; between them tau is refined from E_best + 1, never below the tau
            # carried in
            Tin = Ti.copy()
            for grp in ROUNDS:
                rows = np.array([x for x in grp if 32 * t + x < nd], int)
                if rows.size == 0:
                    continue
                d = 32 * t + rows
                li = np.where(Tin[:, None] >= 0, lt.li_model(np.maximum(Tin, 0)[:, None], V[None, d], widen, rgb=True), -1)
                f = flag[:, rows] & (C[:, d] > li[:, :, None])
                Et = np.where(f, E[:, d], BIG).reshape(nr, -1)
                ct = np.broadcast_to(cidx[:, d], f.shape).reshape(nr, -1)
                k = Et.argmin(1)
                ee, c = Et[np.arange(nr), k], ct[np.arange(nr), k]
                better = (ee < cE) | ((ee == cE) & (c < cc) & (ee != BIG))
                cE, cc = np.where(better, ee, cE), np.where(better, c, cc)
                seen = cE != BIG
                Tin = np.maximum(Tin, np.where(seen, SCALE * st["R"] - n * (np.where(seen, cE, 0) + 1), -1))
            seen = cE != BIG
            th = np.where(seen, theta_update(st["R"], np.where(seen, cE, 1), st["Er"], B, widen), th).astype(F32)
            Ti = np.where(seen, SCALE * st["R"] - n * np.where(seen, cE, 0), -1)
        better = (cE < best_E) | ((cE == best_E) & (cc < best_c))
        best_E, best_c = np.where(better, cE, best_E), np.where(better, cc, best_c)
    return {"E": best_E, "c": best_c, "idx_local": best_c // n_iso, "iso": best_c % n_iso, "exact": exact, "pairs": nr * nd * n_iso}
