"""numpy model of the joint-RGB codec with the 8 isometries of the square, on the unchanged oracle's
building blocks: fo_pool_rgb / fo_range_rgb for the pixels and statistics, fo_iso_source for the index map, fo_java_f2i (through
fo_write_run_rgb) for the quantised rows.  The error of getErrorVarianceCovarianceRGB (FC:760-808) is applied to the explicitly
permuted domain block D_k[i] = D[src_k(i)]: kovarianz_k = sum_i greyR[i] * greyD[src_k(i)] accumulated in float32 in the RANGE
block's order i = 0..n-1, one rounding per add; varianzRange, varianzDomain, varianzSquare (with its quirk) and the channel
means are those of the unpermuted block.  Scan FC:702-715: candidates in window order, k = 0..7 inside a candidate, strict '<'
against 10000000.  Collage (FC:308-347) and decoder (FC:430-508) paint pixel (rx, ry) from the domain pixel at src_k(rx, ry).
With n_iso = 1 all of it is the oracle's fo_encode_rgb / fo_collage_rgb / fo_decode_rgb.  Test infrastructure only."""
import numpy as np

import qtmodel as qm
import qtrgbmodel as qr
from oracle import fic_oracle as fo

F = np.float32


def iso_table(B):
    """int64 [8, B*B]: src_k(i) of fo_iso_source, i = x + y * B."""
    L = fo.lib()
    return np.array([[L.fo_iso_source(k, B, i % B, i // B) for i in range(B * B)] for k in range(8)], np.int64)


def window_globals(w, h, B, wK):
    """int64 [N_r, wK*wK]: pool index of window candidate c of every range block (generateKernel FC:84-100, FC:128-150)."""
    Rw, Rh, Dw, Dh = fo.geometry(w, h, B)
    nr = Rw * Rh
    return np.stack([qm.global_index(w, h, B, wK, np.full(nr, c, np.int32)) for c in range(wK * wK)], axis=1)


def _f2i(v):
    """Java (int) cast of float32 values (NaN -> 0, saturating) as int64."""
    v = np.asarray(v, np.float64)
    return np.where(np.isnan(v), 0, np.clip(np.trunc(np.nan_to_num(v, nan=0.0)), -2147483648, 2147483647)).astype(np.int64)


def encode(argb, w, h, B, wK, n_iso=1, rows=None):
    """dict(info float32 [N_r, 5] = {c, a, bR, bG, bB}, iso int32 [N_r], err float32 [N_r], qrows int32 [N_r, 5]).  `rows`: only
    these range blocks are searched (the others keep zero rows): a sample of a large image."""
    assert n_iso in (1, 8)
    argb = np.ascontiguousarray(argb, np.int32).reshape(-1)
    n = B * B
    pix, dmean, vD = fo.pool_rgb(argb, w, h, B)                       # [N_d, n, 3], [N_d, 3], [N_d]
    greyR, vR = fo.range_rgb(argb, w, h, B)                           # [N_r, n], [N_r]
    nr = greyR.shape[0]
    rmean = qr.blocks(qr.channels(argb, w, h), B).sum(axis=1) // n    # [N_r, 3] rangeRM / GM / BM (FC:771-773)
    greyD = (pix - dmean[:, None, :]).sum(axis=2).astype(F)           # exact small integers
    dev = (pix - dmean[:, None, :]).astype(np.int64)
    varsq = ((dev[:, :, 0] ** 2).sum(axis=1).astype(F) + (dev[:, :, 1] ** 2).sum(axis=1).astype(F)) + dmean[:, 2].astype(F)   # FC:776 (sic)
    src = iso_table(B)[:n_iso]                                        # [K, n]
    G = window_globals(w, h, B, wK)                                   # [N_r, C]
    C, K = G.shape[1], n_iso
    info = np.zeros((nr, 5), F)
    iso = np.zeros(nr, np.int32)
    err = np.zeros(nr, F)
    sel = np.arange(nr) if rows is None else np.asarray(rows, np.int64)
    step = max(1, int(2_000_000 // (C * K)))
    gRf = greyR.astype(F)
    vRf, vDf = vR.astype(F), vD.astype(F)
    for s0 in range(0, sel.size, step):
        js = sel[s0:s0 + step]
        g = G[js]                                                     # [m, C]
        kov = np.zeros((js.size, C, K), F)
        for i in range(n):                                            # the range block's order; one float32 add per step
            d = greyD[g[:, :, None], src[None, None, :, i]]           # [m, C, K]
            kov = kov + gRf[js, i][:, None, None] * d                 # product exact (< 2^24), the add rounds once
        den = vRf[js][:, None] * vDf[g]                               # [m, C]
        zero = (vR[js][:, None] == 0) | (vD[g] == 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(zero[:, :, None], F(0), kov / np.where(zero, F(1), den)[:, :, None]).astype(F)
        r = r * r
        e = ((vRf[js] * vRf[js])[:, None, None] * (F(1) - r)).astype(F)
        flat = e.reshape(js.size, C * K)
        t = np.argmin(flat, axis=1)                                   # first minimum = the lower (c, k): Java's strict '<'
        emin = flat[np.arange(js.size), t]
        won = emin < F(10000000)                                      # FC:702: nothing beats smallestError -> the all-zero row
        c, k = t // K, t % K
        gw = g[np.arange(js.size), c]
        kw = kov[np.arange(js.size), c, k]
        with np.errstate(divide="ignore", invalid="ignore"):
            a = (kw / varsq[gw]).astype(F)                            # FC:718
        a = np.where(a > 1, F(1), a)                                  # FC:721-724 (NaN passes)
        a = np.where(a < -1, F(-1), a).astype(F)
        b = rmean[js].astype(F) - (a[:, None] * dmean[gw].astype(F)).astype(F)
        row = np.concatenate([c.astype(F)[:, None], a[:, None], b.astype(F)], axis=1)
        nan_row = np.array([0, np.nan, np.nan, np.nan, np.nan], F)    # best[] all zero: a = 0 / 0, b = 0 - NaN * 0
        info[js] = np.where(won[:, None], row, nan_row[None, :])
        iso[js] = np.where(won, k, 0)
        err[js] = emin
    return {"info": info, "iso": iso, "err": err, "qrows": fo.quantise_rgb(info)}


def _domain_pixels(scaled, w, h, B, wK, idx_local, iso):
    """int64 [N_r, B*B, 3]: the domain pixel every pixel of every range block is painted from (position x + y*B)."""
    Ws = scaled.shape[1]
    Dw = 2 * (2 * Ws // B) - 3
    ab = B // 4
    gi = qm.global_index(w, h, B, wK, np.asarray(idx_local, np.int32))
    sp = iso_table(B)[np.asarray(iso, np.int64)]                      # [N_r, n] source position of pixel i
    rr = (gi // Dw * ab)[:, None] + sp // B
    cc = (gi % Dw * ab)[:, None] + sp % B
    return scaled[rr, cc]


def _unblock(vals, w, h, B):
    """[N_r, B*B, 3] -> [h, w, 3]."""
    return vals.reshape(h // B, w // B, B, B, 3).transpose(0, 2, 1, 3, 4).reshape(h, w, 3)


def collage(argb, w, h, B, wK, info, iso):
    """getBestGeneratedCollageRGB (FC:308-347) from the unquantised rows: int32 ARGB [h*w]."""
    d = _domain_pixels(qr.scale_rgb(qr.channels(argb, w, h)), w, h, B, wK, info[:, 0].astype(np.int32), iso).astype(F)
    a = info[:, 1].astype(F)
    with np.errstate(invalid="ignore"):
        v = (a[:, None, None] * d).astype(F) + info[:, 2:5].astype(F)[:, None, :]
    return qr.pack(_unblock(np.clip(_f2i(v), 0, 255), w, h, B)).reshape(-1)


def decode(qrows, iso, w, h, B, wK, avg_error_in=0.0):
    """decodeRGB (FC:430-508) from quantised rows and an isometry column: (rgb uint8 [h, w, 3], avgError float32, iterations).
    The paint loop of qtrgbmodel.decode with the domain block permuted by src_k."""
    q = np.asarray(qrows, np.int32).reshape(-1, 5)
    a = q[:, 1].astype(F) / F(1e6)
    b = np.stack([q[:, 2].astype(F) / F(1e5), q[:, 3].astype(F) / F(1e5), q[:, 4].astype(F)], axis=1)
    img = np.full((h, w, 3), 128, np.int64)
    avg = F(avg_error_in)
    iters = 0
    for counter in range(50):
        d = _domain_pixels(qr.scale_rgb(img), w, h, B, wK, q[:, 0], iso).astype(F)
        v = (a[:, None, None] * d).astype(F) + b[:, None, :]          # two roundings, never fused
        vals = np.clip(np.trunc(v).astype(np.int64), 0, 255)
        diff = qr.blocks(img, B) - vals
        sq = (diff * diff).sum(axis=-1).reshape(-1)                   # Java's visiting order: block by block, rows inside
        img = _unblock(vals, w, h, B)
        acc = np.add.accumulate(np.concatenate([[avg], sq.astype(F)]).astype(F), dtype=F)
        avg = F(acc[-1] / F(w * h))
        iters = counter + 1
        if avg < 1:
            break
        if counter != 49:
            avg = F(0.0)
    return img.astype(np.uint8), F(avg), iters
