"""numpy int64 model of the least-squares domain search of the joint-RGB path: for every range block
the candidate (window block, isometry) whose QUANTISED map {qa / 1000, t_R / 100, t_G / 100, t_B} -- one a for the three
channels, three b -- has the smallest squared error, everything in exact integers.  From the oracle only the pool
(createCodebuchRGB through fo.pool_rgb), fo_iso_source and the window indices (calculateIndices) are taken, as lsqmodel.py does;
the search itself is restated here.  Test infrastructure only.

Per range block r and candidate d (pool block g read through isometry k), n = B*B, per channel ch the sums S_r, S_rr, S_d, S_dd,
S_rd = sum r d_k:
  C = sum_ch (n S_rd - S_r S_d),  V = sum_ch (n S_dd - S_d^2)
  qa  = 0 if V == 0 else clamp(floor((2000 C + V) / (2 V)), -1000, 1000)
  t_R, t_G = floor((2 (1000 S_r - qa S_d) + 10 n) / (20 n)),   t_B = floor((2 (1000 S_r - qa S_d) + 1000 n) / (2000 n))
  u_R = 10 t_R, u_G = 10 t_G, u_B = 1000 t_B
  E = sum_ch (10^6 S_rr + qa^2 S_dd + n u^2 - 2000 qa S_rd - 2000 u S_r + 2 qa u S_d) = sum_ch sum_i (1000 r - qa d - u_ch)^2
The winner is the smallest E, the first one in the order c = wloc * n_iso + k.  Only the channel sums of S_rr, S_dd and S_rd
enter, so the search needs one dot product over the 3 n bytes of a block."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import fic_oracle as fo

import qtmodel
import qtrgbmodel as qr

I64 = np.int64


def fit(n, S_r, S_d, S_dd, S_rd):
    """(qa, t [..., 3]) of the definition on int64 arrays: S_r, S_d [..., 3] per channel, S_dd and S_rd summed over the
    channels.  numpy's // on integers is the mathematical floor."""
    S_r, S_d, S_dd, S_rd = (np.asarray(x, I64) for x in (S_r, S_d, S_dd, S_rd))
    C = n * S_rd - (S_r * S_d).sum(axis=-1)
    V = n * S_dd - (S_d * S_d).sum(axis=-1)
    qa = np.where(V == 0, 0, np.clip((2000 * C + V) // np.where(V == 0, 1, 2 * V), -1000, 1000))
    m = 2 * (1000 * S_r - qa[..., None] * S_d)
    t = np.stack([(m[..., 0] + 10 * n) // (20 * n), (m[..., 1] + 10 * n) // (20 * n), (m[..., 2] + 1000 * n) // (2000 * n)], axis=-1)
    return qa, t


def _u(t):
    return np.asarray(t, I64) * np.array([10, 10, 1000], I64)


def closed_form(n, S_r, S_rr, S_d, S_dd, S_rd, qa, t):
    """E of the definition from the sums, int64 (S_rr, S_dd, S_rd summed over the channels)."""
    S_r, S_rr, S_d, S_dd, S_rd, qa = (np.asarray(x, I64) for x in (S_r, S_rr, S_d, S_dd, S_rd, qa))
    u = _u(t)
    return (1000000 * S_rr + qa * qa * S_dd - 2000 * qa * S_rd
            + (n * u * u - 2000 * u * S_r + 2 * qa[..., None] * u * S_d).sum(axis=-1))


def direct_sum(r, d, qa, t):
    """sum_ch sum_i (1000 r - qa d - u_ch)^2 of r, d [..., n, 3]: what closed_form must equal."""
    r, d = np.asarray(r, I64), np.asarray(d, I64)
    e = 1000 * r - np.asarray(qa, I64)[..., None, None] * d - _u(t)[..., None, :]
    return (e * e).sum(axis=(-1, -2))


def _flat(argb):
    return np.ascontiguousarray(argb, np.int32).reshape(-1)


def _pool(argb, w, h, B):
    return fo.pool_rgb(_flat(argb), w, h, B)[0].astype(I64)                 # [N_d, n, 3]


def window_globals(w, h, B, wK):
    """int64 [N_r, wK*wK]: pool index of every window-local candidate of every range block (calculateIndices)."""
    nr = (w // B) * (h // B)
    return np.stack([qtmodel.global_index(w, h, B, wK, np.full(nr, wloc, np.int32)) for wloc in range(wK * wK)], axis=1)


def rows_of(wloc, qa, t):
    """The stream rows {idx_local, 1000 qa, 1000 t_R, 1000 t_G, t_B} (int32 [N, 5])."""
    wloc, qa, t = np.asarray(wloc, I64), np.asarray(qa, I64), np.asarray(t, I64)
    return np.stack([wloc, 1000 * qa, 1000 * t[:, 0], 1000 * t[:, 1], t[:, 2]], axis=1).astype(np.int32)


def coefs(qrows):
    """a, bR, bG, bB (float32) the decoder makes of the rows: (float) q1 / 1e6f, (float) q2 / 1e5f, (float) q3 / 1e5f, (float) q4."""
    q = np.asarray(qrows, np.int32)
    f = np.float32
    return (q[:, 1].astype(f) / f(1e6), q[:, 2].astype(f) / f(1e5), q[:, 3].astype(f) / f(1e5), q[:, 4].astype(f))


def encode(argb, w, h, B, wK=None, n_iso=1, budget=1 << 21):
    """The least-squares codebook of the packed ARGB image: dict of [N_r] arrays idx_local, idx_global, iso (int32), qrows int32
    [N_r, 5], E int64, a / bR / bG / bB float32 as the library returns them.  wK = None: full search."""
    assert n_iso in (1, 8)
    Rw, Rh, Dw, Dh = fo.geometry(w, h, B)
    wK = Dw if wK is None else wK
    n = B * B
    pix = _pool(argb, w, h, B)
    full = wK == Dw and wK == Dh
    r = qr.blocks(qr.channels(argb, w, h), B)                                # [N_r, n, 3]
    nr = r.shape[0]
    Sd_all, Sdd_all = pix.sum(axis=1), (pix * pix).sum(axis=(1, 2))          # [N_d, 3], [N_d]
    S_r, S_rr = r.sum(axis=1), (r * r).sum(axis=(1, 2))                      # [N_r, 3], [N_r]
    gi_all = None if full else window_globals(w, h, B, wK)
    nw = wK * wK
    iso = qtmodel.iso_table(B)[:n_iso]
    pixk = None
    if full:   # float64 products of bytes summed over 3 n <= 768 positions stay below 2^53: the matmul is exact
        pixk = np.stack([pix[:, iso[k], :] for k in range(n_iso)], axis=1).astype(np.float64).reshape(-1, 3 * n)
    best_c, best_E, best_qa = (np.zeros(nr, I64) for _ in range(3))
    best_t = np.zeros((nr, 3), I64)
    step = max(1, budget // (nw * n_iso))

    def chunk(j0):
        rr = r[j0:j0 + step]
        m = rr.shape[0]
        if full:
            S_rd = np.rint(rr.reshape(m, 3 * n).astype(np.float64) @ pixk.T).astype(I64).reshape(m, nw, n_iso)
            S_d, S_dd = Sd_all[None, :, None, :], Sdd_all[None, :, None]
        else:
            gi = gi_all[j0:j0 + m]
            d = pix[gi][:, :, iso, :]                                                            # [m, nw, n_iso, n, 3]
            S_rd = (rr[:, None, None, :, :] * d).sum(axis=(-1, -2))
            S_d, S_dd = Sd_all[gi][:, :, None, :], Sdd_all[gi][:, :, None]
        sr, srr = S_r[j0:j0 + m, None, None, :], S_rr[j0:j0 + m, None, None]
        qa, t = fit(n, sr, S_d, S_dd, S_rd)
        E = closed_form(n, sr, srr, S_d, S_dd, S_rd, qa, t).reshape(m, -1)
        c = E.argmin(axis=1)                                   # the first minimum: strict '<' in candidate order
        rows = np.arange(m)
        return j0, m, c, E[rows, c], qa.reshape(m, -1)[rows, c], t.reshape(m, -1, 3)[rows, c]

    # the chunks are independent and numpy drops the GIL inside its loops: a few threads, whatever the machine has
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        for j0, m, c, E, qa, t in pool.map(chunk, range(0, nr, step)):
            best_c[j0:j0 + m], best_E[j0:j0 + m], best_qa[j0:j0 + m], best_t[j0:j0 + m] = c, E, qa, t
    wloc, k = best_c // n_iso, best_c % n_iso
    gidx = wloc if full else gi_all[np.arange(nr), wloc]
    qrows = rows_of(wloc, best_qa, best_t)
    a, bR, bG, bB = coefs(qrows)
    return {"idx_local": wloc.astype(np.int32), "idx_global": gidx.astype(np.int32), "iso": k.astype(np.int32), "qrows": qrows,
            "E": best_E, "a": a, "bR": bR, "bG": bG, "bB": bB, "wK": wK}


def rows_error(argb, w, h, B, wK, qrows, iso=None):
    """int64 [N_r]: sum_ch sum_i (1000 r - q1 d / 1000 - u)^2 of ANY quantised rows {idx_local, q1, q2, q3, q4} + isometries on
    the grids of the stream (a = q1 / 10^6, bR = q2 / 10^5, bG = q3 / 10^5, bB = q4), times 10^6 like E; the rows of this search
    lie on the coarser grids exactly, so it returns their E.  Evaluated in float64 where a row is off those grids (the
    reference's rows): a yardstick for comparing sums, not a bit-exact quantity there."""
    Dw = fo.geometry(w, h, B)[2]
    wK = Dw if wK is None else wK
    q = np.asarray(qrows, I64)
    iso = np.zeros(q.shape[0], I64) if iso is None else np.asarray(iso, I64)
    gi = qtmodel.global_index(w, h, B, wK, q[:, 0].astype(np.int32))
    d = _pool(argb, w, h, B)[gi[:, None], qtmodel.iso_table(B)[iso]]        # [N_r, n, 3]
    r = qr.blocks(qr.channels(argb, w, h), B)
    on_grid = (q[:, 1] % 1000 == 0).all() and (q[:, 2] % 1000 == 0).all() and (q[:, 3] % 1000 == 0).all()
    if on_grid:
        return direct_sum(r, d, q[:, 1] // 1000, np.stack([q[:, 2] // 1000, q[:, 3] // 1000, q[:, 4]], axis=1))
    u = np.stack([q[:, 2] / 100.0, q[:, 3] / 100.0, q[:, 4] * 1000.0], axis=1)
    e = 1000.0 * r - (q[:, 1] / 1000.0)[:, None, None] * d - u[:, None, :]
    return (e * e).sum(axis=(1, 2))


def codebooks(argb, w, h, B_max, B_min, wK=0, n_iso=1):
    """{B: (qrows5, iso)} of every quadtree level from the least-squares search: isostreammodel.encode(cbs=...)'s argument
    (qtrgbmodel.encode(cbs=...) takes the qrows5 alone)."""
    out = {}
    for B in qtmodel.levels(B_max, B_min):
        r = encode(argb, w, h, B, qtmodel.level_wk(w, h, B, wK), n_iso)
        out[B] = (r["qrows"], r["iso"])
    return out
