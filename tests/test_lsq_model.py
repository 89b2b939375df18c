"""Least-squares domain search, CPU side: the numpy int64 model (tests/lsqmodel.py) against its own
definition, and the quality it buys on LenaGrey -- fixed block sizes through the oracle's decode_rows, the quadtree through
tests/qtmodel.py with the per-level codebooks swapped."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lsqmodel as lm  # noqa: E402
import qtmodel as qm  # noqa: E402

SETTINGS = [(B, k) for B in (4, 8, 16) for k in (1, 8)]
# decode PSNR in dB on lena_grey_256.npy, full search: {(B, n_iso): (reference criterion, least squares)}
PSNR = {(4, 1): (27.18, 31.06), (4, 8): (27.26, 32.35), (8, 1): (24.82, 25.80), (8, 8): (24.89, 26.40),
        (16, 1): (22.07, 22.34), (16, 8): (22.79, 23.13)}
# quadtree 16 -> 4, wK = 0: {(n_iso, threshold): ((leaves, dB) reference criterion, (leaves, dB) least squares)}
QT = {(1, 400.0): ((937, 24.87), (874, 26.04)), (1, 100.0): ((1747, 26.51), (1690, 29.40)),
      (8, 400.0): ((859, 25.14), (787, 26.54)), (8, 100.0): ((1624, 26.67), (1552, 30.12))}


def test_closed_form_equals_direct_sum():
    rng = np.random.RandomState(19)
    for B in (4, 8, 16):
        n = B * B
        r = rng.randint(0, 256, size=(4000, n)).astype(np.int64)
        d = rng.randint(0, 256, size=(4000, n)).astype(np.int64)
        d[:500] = rng.randint(0, 256, size=(500, 1))                    # flat domains: V == 0
        d[500:1200] = rng.randint(100, 104, size=(700, n))              # low contrast: qa clamps at +-100
        r[500:1200] = rng.choice([0, 255], size=(700, n))
        d[1200:1900] = 255 - r[1200:1900] // 2                          # negative slopes
        d[1900:2200] = rng.randint(0, 256, size=(300, n))               # dark ranges, small positive slopes: qb below 0
        r[1900:2200] = d[1900:2200] // 128
        S_r, S_rr, S_d, S_dd, S_rd = r.sum(1), (r * r).sum(1), d.sum(1), (d * d).sum(1), (r * d).sum(1)
        qa, qb = lm.fit(n, S_r, S_d, S_dd, S_rd)
        C, V = n * S_rd - S_r * S_d, n * S_dd - S_d * S_d
        assert (V == 0).sum() >= 500 and (qa[V == 0] == 0).all()
        assert (qa == 100).sum() >= 50 and (qa == -100).sum() >= 50
        neg = (200 * C + V < 0) & (V > 0)
        assert neg.sum() >= 500 and ((200 * C + V)[neg] % (2 * V[neg]) != 0).sum() >= 400      # floor differs from truncation
        assert (2 * (100 * S_r - qa * S_d) + 100 * n < 0).sum() >= 50
        # nearest: |100 C / V - qa| <= 1/2 where unclamped, |mean_r - qa mean_d / 100 - qb| <= 1/2
        un = (V > 0) & (np.abs(qa) < 100)
        assert (np.abs(200 * C[un] - 2 * qa[un] * V[un]) <= V[un]).all()
        assert (np.abs(2 * (100 * S_r - qa * S_d) - 200 * n * qb) <= 100 * n).all()
        E = lm.closed_form(n, S_r, S_rr, S_d, S_dd, S_rd, qa, qb)
        assert (E == lm.direct_sum(r, d, qa, qb)).all() and (E >= 0).all()


@pytest.fixture(scope="module")
def lena_lsq(lena_grey, oracle):
    return {(B, k): lm.encode(lena_grey, B, None, k) for B, k in SETTINGS}


@pytest.fixture(scope="module")
def lena_ref(lena_grey, oracle):
    h, w = lena_grey.shape
    argb = oracle.gray_to_argb(lena_grey)
    out = {}
    for B, k in SETTINGS:
        r = oracle.encode_gray(argb, w, h, B, oracle.geometry(w, h, B)[2], k)
        out[(B, k)] = (oracle.quantise_gray(r["info"]), r["iso"].astype(np.int32))
    return out


@pytest.mark.parametrize("B,n_iso", SETTINGS)
def test_decode_psnr_lena(lena_grey, lena_lsq, lena_ref, oracle, B, n_iso):
    h, w = lena_grey.shape
    wK = oracle.geometry(w, h, B)[2]
    ref = oracle.psnr(oracle.decode_rows(*lena_ref[(B, n_iso)], w, h, B, wK)[0], lena_grey)
    r = lena_lsq[(B, n_iso)]
    lsq = oracle.psnr(oracle.decode_rows(r["qrows"], r["iso"], w, h, B, wK)[0], lena_grey)
    print(f"B={B} n_iso={n_iso}: reference {ref:.3f} dB, least squares {lsq:.3f} dB")
    assert abs(ref - PSNR[(B, n_iso)][0]) <= 0.01 and abs(lsq - PSNR[(B, n_iso)][1]) <= 0.01


@pytest.mark.parametrize("B,n_iso", SETTINGS)
def test_total_error_below_reference_rows_lena(lena_grey, lena_lsq, lena_ref, B, n_iso):
    r = lena_lsq[(B, n_iso)]
    assert (r["E"] == lm.rows_error(lena_grey, B, None, r["qrows"], r["iso"])).all()
    assert r["E"].sum() < lm.rows_error(lena_grey, B, None, *lena_ref[(B, n_iso)]).sum()


@pytest.mark.parametrize("B,n_iso", SETTINGS)
def test_total_error_below_reference_rows_lena64(lena64, oracle, B, n_iso):
    h, w = lena64.shape
    ref = oracle.encode_gray(oracle.gray_to_argb(lena64), w, h, B, oracle.geometry(w, h, B)[2], n_iso)
    r = lm.encode(lena64, B, None, n_iso)
    assert (r["E"] == lm.rows_error(lena64, B, None, r["qrows"], r["iso"])).all()
    assert r["E"].sum() < lm.rows_error(lena64, B, None, oracle.quantise_gray(ref["info"]), ref["iso"]).sum()


@pytest.mark.parametrize("wK", [1, 3])
def test_windowed_search_is_the_exhaustive_minimum(lena64, oracle, wK):
    """The windowed path of the model against a plain loop over the window on a few range blocks."""
    B, n_iso = 8, 8
    h, w = lena64.shape
    r = lm.encode(lena64, B, wK, n_iso)
    gi = lm.window_globals(w, h, B, wK)
    pix = oracle.pool(oracle.gray_to_argb(lena64), w, h, B)[0].astype(np.int64)
    blk = qm.blocks(lena64, B)
    for j in (0, 7, 35, 63):
        best = None
        for wloc in range(wK * wK):
            for k in range(n_iso):
                d = pix[gi[j, wloc]][qm.iso_table(B)[k]]
                qa, qb = lm.fit(B * B, blk[j].sum(), d.sum(), (d * d).sum(), (blk[j] * d).sum())
                E = int(lm.direct_sum(blk[j], d, qa, qb))
                if best is None or E < best[0]:
                    best = (E, wloc, k, int(qa), int(qb))
        assert best == (int(r["E"][j]), int(r["idx_local"][j]), int(r["iso"][j]), int(r["qrows"][j, 1]), int(r["qrows"][j, 2]))


@pytest.mark.parametrize("n_iso,threshold", sorted(QT))
def test_quadtree_leaves_and_psnr_lena(lena_grey, lena_lsq, lena_ref, n_iso, threshold):
    h, w = lena_grey.shape
    for which, cbs in ((0, {B: lena_ref[(B, n_iso)] for B in (16, 8, 4)}),
                       (1, {B: (lena_lsq[(B, n_iso)]["qrows"], lena_lsq[(B, n_iso)]["iso"]) for B in (16, 8, 4)})):
        leaves = qm.encode(lena_grey, 16, 4, 0, n_iso, threshold, cbs)
        run = qm.write_run(leaves, w, h, 16, 4, 0, n_iso)
        db = 10.0 * np.log10(255.0 ** 2 / np.mean((qm.decode(run)[0].astype(np.float64) - lena_grey) ** 2))
        want = QT[(n_iso, threshold)][which]
        print(f"n_iso={n_iso} threshold={threshold} {('reference', 'least squares')[which]}: {len(leaves)} leaves, {len(run)} B, {db:.3f} dB")
        assert len(leaves) == want[0] and abs(db - want[1]) <= 0.01
