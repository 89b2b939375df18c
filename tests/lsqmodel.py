"""numpy int64 model of the least-squares domain search: for every range block the candidate (window
block, isometry) whose QUANTISED affine map {qa / 100, qb} has the smallest squared error, everything in exact integers.  From
the oracle only the pool (createCodebuch), fo_iso_source and the window indices (calculateIndices) are taken, as qtmodel.py
does; the search itself is restated here.  Test infrastructure only.

Per range block r and candidate d (pool block g read through isometry k), n = B*B:
  S_r = sum r, S_rr = sum r^2, S_d = sum d, S_dd = sum d^2, S_rd = sum r d_k
  C = n S_rd - S_r S_d,  V = n S_dd - S_d^2
  qa = 0 if V == 0 else clamp(floor((200 C + V) / (2 V)), -100, 100)
  qb = floor((2 (100 S_r - qa S_d) + 100 n) / (200 n))
  E  = 10^4 S_rr + qa^2 S_dd + 10^4 n qb^2 - 200 qa S_rd - 2 10^4 qb S_r + 200 qa qb S_d  =  sum (100 r - qa d - 100 qb)^2
The winner is the smallest E, the first one in the order c = wloc * n_iso + k."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import fic_oracle as fo

import qtmodel

I64 = np.int64


def fit(n, S_r, S_d, S_dd, S_rd):
    """(qa, qb) of the definition, elementwise on int64 arrays.  numpy's // on integers is the mathematical floor."""
    S_r, S_d, S_dd, S_rd = (np.asarray(x, I64) for x in (S_r, S_d, S_dd, S_rd))
    C = n * S_rd - S_r * S_d
    V = n * S_dd - S_d * S_d
    qa = np.where(V == 0, 0, np.clip((200 * C + V) // np.where(V == 0, 1, 2 * V), -100, 100))
    qb = (2 * (100 * S_r - qa * S_d) + 100 * n) // (200 * n)
    return qa, qb


def closed_form(n, S_r, S_rr, S_d, S_dd, S_rd, qa, qb):
    """E of the definition from the five sums, int64."""
    S_r, S_rr, S_d, S_dd, S_rd, qa, qb = (np.asarray(x, I64) for x in (S_r, S_rr, S_d, S_dd, S_rd, qa, qb))
    return (10000 * S_rr + qa * qa * S_dd + 10000 * n * qb * qb - 200 * qa * S_rd - 20000 * qb * S_r + 200 * qa * qb * S_d)


def direct_sum(r, d, qa, qb):
    """sum (100 r - qa d - 100 qb)^2 over the last axis: what closed_form must equal."""
    r, d = np.asarray(r, I64), np.asarray(d, I64)
    t = 100 * r - np.asarray(qa, I64)[..., None] * d - 100 * np.asarray(qb, I64)[..., None]
    return (t * t).sum(axis=-1)


def _pool(gray, B):
    h, w = gray.shape
    return fo.pool(fo.gray_to_argb(gray), w, h, B)[0].astype(I64)


def window_globals(w, h, B, wK):
    """int64 [N_r, wK*wK]: pool index of every window-local candidate of every range block (calculateIndices)."""
    nr = (w // B) * (h // B)
    return np.stack([qtmodel.global_index(w, h, B, wK, np.full(nr, wloc, np.int32)) for wloc in range(wK * wK)], axis=1)


def encode(gray, B, wK=None, n_iso=1, budget=1 << 21):
    """The least-squares codebook of `gray` (uint8 [H, W]): dict of [N_r] arrays idx_local, idx_global, iso (int32), qrows int32
    [N_r, 3], E int64, a / b / err float32 as the library returns them.  wK = None: full search."""
    gray = np.ascontiguousarray(gray, np.uint8)
    h, w = gray.shape
    Rw, Rh, Dw, Dh = fo.geometry(w, h, B)
    wK = Dw if wK is None else wK
    n = B * B
    pix = _pool(gray, B)
    full = wK == Dw and wK == Dh
    r = qtmodel.blocks(gray, B)
    nr = r.shape[0]
    Sd_all, Sdd_all = pix.sum(axis=1), (pix * pix).sum(axis=1)
    S_r, S_rr = r.sum(axis=1), (r * r).sum(axis=1)
    gi_all = None if full else window_globals(w, h, B, wK)
    nw = wK * wK
    iso = qtmodel.iso_table(B)[:n_iso]
    pixk = None
    if full:   # float64 products of bytes summed over n <= 256 positions stay below 2^53: the matmul is exact
        pixk = np.stack([pix[:, iso[k]] for k in range(n_iso)], axis=1).astype(np.float64)      # [N_d, n_iso, n]
    best_c, best_E, best_qa, best_qb = (np.zeros(nr, I64) for _ in range(4))
    step = max(1, budget // (nw * n_iso))

    def chunk(j0):
        rr = r[j0:j0 + step]
        m = rr.shape[0]
        if full:
            S_rd = np.rint(rr.astype(np.float64) @ pixk.reshape(-1, n).T).astype(I64).reshape(m, nw, n_iso)
            S_d, S_dd = Sd_all[None, :, None], Sdd_all[None, :, None]
        else:
            gi = gi_all[j0:j0 + m]
            d = pix[gi][:, :, iso]                                                               # [m, nw, n_iso, n]
            S_rd = (rr[:, None, None, :] * d).sum(axis=-1)
            S_d, S_dd = Sd_all[gi][:, :, None], Sdd_all[gi][:, :, None]
        sr, srr = S_r[j0:j0 + m, None, None], S_rr[j0:j0 + m, None, None]
        qa, qb = fit(n, sr, S_d, S_dd, S_rd)
        E = closed_form(n, sr, srr, S_d, S_dd, S_rd, qa, qb).reshape(m, -1)
        c = E.argmin(axis=1)                                   # the first minimum: strict '<' in candidate order
        rows = np.arange(m)
        pick = lambda q: np.broadcast_to(q, (m, nw, n_iso)).reshape(m, -1)[rows, c]
        return j0, m, c, E[rows, c], pick(qa), pick(qb)

    # the chunks are independent and numpy drops the GIL inside its loops: a few threads, whatever the machine has
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        for j0, m, c, E, qa, qb in pool.map(chunk, range(0, nr, step)):
            best_c[j0:j0 + m], best_E[j0:j0 + m], best_qa[j0:j0 + m], best_qb[j0:j0 + m] = c, E, qa, qb
    wloc, k = best_c // n_iso, best_c % n_iso
    gidx = wloc if full else gi_all[np.arange(nr), wloc]
    return {"idx_local": wloc.astype(np.int32), "idx_global": gidx.astype(np.int32), "iso": k.astype(np.int32),
            "qrows": np.stack([wloc, best_qa, best_qb], axis=1).astype(np.int32), "E": best_E,
            "a": (best_qa.astype(np.float32) / np.float32(100.0)).astype(np.float32), "b": best_qb.astype(np.float32),
            "err": (best_E.astype(np.float64) / 1e4).astype(np.float32), "wK": wK}


def rows_error(gray, B, wK, qrows, iso):
    """int64 [N_r]: E of the given quantised rows {idx_local, qa, qb} + isometries, by the direct sum."""
    gray = np.ascontiguousarray(gray, np.uint8)
    h, w = gray.shape
    Dw = fo.geometry(w, h, B)[2]
    wK = Dw if wK is None else wK
    q = np.asarray(qrows, I64)
    gi = qtmodel.global_index(w, h, B, wK, q[:, 0].astype(np.int32))
    d = _pool(gray, B)[gi[:, None], qtmodel.iso_table(B)[np.asarray(iso, I64)]]
    return direct_sum(qtmodel.blocks(gray, B), d, q[:, 1], q[:, 2])


def codebooks(gray, B_max, B_min, wK=0, n_iso=1):
    """{B: (qrows, iso)} of every quadtree level from the least-squares search: qtmodel.encode(cbs=...)'s argument."""
    h, w = gray.shape
    out = {}
    for B in qtmodel.levels(B_max, B_min):
        r = encode(gray, B, qtmodel.level_wk(w, h, B, wK), n_iso)
        out[B] = (r["qrows"], r["iso"])
    return out
