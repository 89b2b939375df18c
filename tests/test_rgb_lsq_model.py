"""Least-squares domain search of the joint-RGB path, CPU side: the numpy int64 model
(tests/rgblsqmodel.py) against its own definition, the quality it buys on LenaColored -- fixed block sizes through
rgbisomodel.decode, the quadtree through qtrgbmodel / isostreammodel with the per-level codebooks swapped -- the host check of
the kernels' fit (tests/cpp/lsq_rgb_fit_test.cpp) and the refusals of the new entries that need no device."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isostreammodel as im  # noqa: E402
import qtmodel as qm  # noqa: E402
import qtrgbmodel as qr  # noqa: E402
import rgbisomodel as rim  # noqa: E402
import rgblsqmodel as lm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = H = 256
# B = 4 with 8 isometries is 5e8 pairs in numpy: the model gives 33.30 dB, 7 iterations, sum E 5 404 984 219 170 there, and no test pins them
SETTINGS = [(4, 1), (8, 1), (8, 8), (16, 1), (16, 8)]
# on lena_colored_256.npy, full search: {(B, n_iso): (decode PSNR in dB and iterations of the reference criterion's rows, of the
# least-squares rows, sum of E over the least-squares rows)}
LENA = {(4, 1): ((21.81, 15), (32.30, 7), 6726817313993), (8, 1): ((20.11, 12), (26.83, 8), 24014909343832),
        (8, 8): ((20.63, 11), (27.41, 8), 20754553723364), (16, 1): ((18.53, 13), (22.92, 8), 61423690635641),
        (16, 8): ((18.29, 12), (23.52, 8), 53743567805500)}
# quadtree from 16 down, wK = 0: {(tag, n_iso, B_min, threshold): ((leaves, stream bytes, dB) reference criterion, the same of
# least squares)}.  Tag 3 (qtrgbmodel, 24 bytes a leaf) and tag 6 (isostreammodel, 28 bytes a leaf) with one isometry go 16 -> 4;
# with 8 isometries the tree stops at 8 (B = 4 with 8 isometries: see SETTINGS).  DESIGN.md 4.14 has the reference's figures.
QT = {(3, 1, 4, 1200.0): ((1759, 42248, 21.52), (778, 18704, 26.26)), (3, 1, 4, 600.0): ((2332, 56000, 21.80), (1201, 28856, 28.23)),
      (6, 1, 4, 1200.0): ((1759, 49284, 21.52), (778, 21816, 26.26)), (6, 1, 4, 600.0): ((2332, 65328, 21.80), (1201, 33660, 28.23)),
      (6, 8, 8, 1200.0): ((775, 21732, 20.38), (460, 12912, 25.57)), (6, 8, 8, 600.0): ((868, 24336, 20.56), (574, 16104, 26.38))}


def test_closed_form_equals_direct_sum():
    rng = np.random.RandomState(20)
    for B in (4, 8, 16):
        n = B * B
        r = rng.randint(0, 256, size=(4000, n, 3)).astype(np.int64)
        d = rng.randint(0, 256, size=(4000, n, 3)).astype(np.int64)
        d[:500] = rng.randint(0, 256, size=(500, 1, 3))                 # flat domains: V == 0
        d[500:1200] = rng.randint(100, 104, size=(700, n, 3))           # low contrast: qa clamps at +-1000
        r[500:1200] = rng.choice([0, 255], size=(700, n, 3))
        d[1200:1900] = 255 - r[1200:1900] // 2                          # negative slopes
        d[1900:2600] = rng.randint(0, 256, size=(700, n, 3))            # convex in d: intercepts below 0 in every channel
        r[1900:2600] = d[1900:2600] ** 2 // 1020
        S_r, S_d = r.sum(1), d.sum(1)
        S_rr, S_dd, S_rd = (r * r).sum((1, 2)), (d * d).sum((1, 2)), (r * d).sum((1, 2))
        qa, t = lm.fit(n, S_r, S_d, S_dd, S_rd)
        C, V = n * S_rd - (S_r * S_d).sum(1), n * S_dd - (S_d * S_d).sum(1)
        assert (V == 0).sum() >= 500 and (qa[V == 0] == 0).all()
        assert (qa == 1000).sum() >= 50 and (qa == -1000).sum() >= 50
        neg = (2000 * C + V < 0) & (V > 0)
        assert neg.sum() >= 500 and ((2000 * C + V)[neg] % (2 * V[neg]) != 0).sum() >= 400     # floor differs from truncation
        assert ((t < 0).sum(0) >= 50).all()                              # t_R, t_G and t_B
        # nearest: |1000 C / V - qa| <= 1/2 where unclamped, |100 (mean_r - a mean_d) - t| <= 1/2 (R, G), |mean_r - a mean_d - t_B| <= 1/2
        un = (V > 0) & (np.abs(qa) < 1000)
        assert (np.abs(2000 * C[un] - 2 * qa[un] * V[un]) <= V[un]).all()
        m = 2 * (1000 * S_r - qa[:, None] * S_d)
        assert (np.abs(m[:, :2] - 20 * n * t[:, :2]) <= 10 * n).all() and (np.abs(m[:, 2] - 2000 * n * t[:, 2]) <= 1000 * n).all()
        E = lm.closed_form(n, S_r, S_rr, S_d, S_dd, S_rd, qa, t)
        assert (E == lm.direct_sum(r, d, qa, t)).all() and (E >= 0).all() and (E < 2 ** 50).all()


def test_kernel_fit_against_plain_int64_host_program(tmp_path):
    """lsq_fit_rgb (csrc/fic_lsq_rgb_fit.h), the fit every kernel of the search calls, as a stand-alone host program: 21 600
    pairs -- among them blocks of 0 and 255 whose V and |C| pass 2^31 at B = 16 -- against the definition in plain 64-bit
    integers and the direct sum, built with AddressSanitizer and
    UndefinedBehaviorSanitizer where the host compiler has them; without them otherwise, and the test prints which of the two
    ran, so a pass on a machine without the runtimes is not read as a sanitizer pass.  Nothing of the program is loaded
    into this process, and it never runs on a GPU."""
    src = os.path.join(ROOT, "tests", "cpp", "lsq_rgb_fit_test.cpp")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    ok = subprocess.run(["g++"] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode == 0
    if not ok or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        san = []
    print("lsq_rgb_fit_test built " + ("with " + san[0] if san else "WITHOUT sanitizers (the host compiler has no runtimes for them)"))
    exe = str(tmp_path / "lsq_rgb_fit_test")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + san + [src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "\n0 failures" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr


def test_windowed_model_against_a_plain_loop(oracle):
    """The vectorised model (windowed and full) against a Python loop over every candidate, on a 32 x 32 image."""
    w = h = 32
    rgb = np.random.RandomState(5).randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    rgb[8:16, 8:24] = (40, 200, 90)                                     # flat blocks among the noise
    argb = oracle.rgb_to_argb(rgb)
    for B, wK, n_iso in ((8, 3, 8), (4, 5, 1), (8, None, 8), (16, None, 8)):
        r = lm.encode(argb, w, h, B, wK, n_iso)
        Dw = oracle.geometry(w, h, B)[2]
        wk = Dw if wK is None else wK
        gi = lm.window_globals(w, h, B, wk)
        pix = oracle.pool_rgb(argb, w, h, B)[0].astype(np.int64)
        blk = qr.blocks(qr.channels(argb, w, h), B)
        iso = qm.iso_table(B)
        for j in range(blk.shape[0]):
            best = None
            for wloc in range(wk * wk):
                for k in range(n_iso):
                    d = pix[gi[j, wloc]][iso[k]]
                    qa, t = lm.fit(B * B, blk[j].sum(0), d.sum(0), (d * d).sum(), (blk[j] * d).sum())
                    E = int(lm.direct_sum(blk[j], d, qa, t))
                    if best is None or E < best[0]:
                        best = (E, wloc, k, 1000 * int(qa), 1000 * int(t[0]), 1000 * int(t[1]), int(t[2]))
            assert best == (int(r["E"][j]), int(r["idx_local"][j]), int(r["iso"][j]), *(int(v) for v in r["qrows"][j, 1:])), (B, wK, j)
            assert int(r["idx_global"][j]) == int(gi[j, r["idx_local"][j]])


@pytest.fixture(scope="module")
def lena_argb(lena_colored, oracle):
    return oracle.rgb_to_argb(lena_colored)


@pytest.fixture(scope="module")
def lena_lsq(lena_argb):
    return {(B, k): lm.encode(lena_argb, W, H, B, None, k) for B, k in SETTINGS}


@pytest.fixture(scope="module")
def lena_ref(lena_argb, oracle):
    out = {}
    for B, k in SETTINGS:
        r = rim.encode(lena_argb, W, H, B, oracle.geometry(W, H, B)[2], k)
        out[(B, k)] = (r["qrows"], r["iso"].astype(np.int32))
    return out


@pytest.mark.parametrize("B,n_iso", SETTINGS)
def test_total_error_and_decode_psnr_lena(lena_colored, lena_argb, lena_lsq, lena_ref, oracle, B, n_iso):
    wK = oracle.geometry(W, H, B)[2]
    r = lena_lsq[(B, n_iso)]
    want_ref, want_lsq, want_E = LENA[(B, n_iso)]
    assert (r["E"] == lm.rows_error(lena_argb, W, H, B, None, r["qrows"], r["iso"])).all()
    total = int(r["E"].sum())
    ref_total = float(lm.rows_error(lena_argb, W, H, B, None, *lena_ref[(B, n_iso)]).sum())
    dec = rim.decode(r["qrows"], r["iso"], W, H, B, wK)
    old = rim.decode(*lena_ref[(B, n_iso)], W, H, B, wK)
    db, db_old = oracle.psnr(dec[0], lena_colored), oracle.psnr(old[0], lena_colored)
    print(f"B={B} n_iso={n_iso}: reference {db_old:.3f} dB ({old[2]} iterations, sum E {ref_total:.6g}), "
          f"least squares {db:.3f} dB ({dec[2]} iterations, sum E {total})")
    assert total == want_E
    assert total < ref_total
    assert abs(db - want_lsq[0]) <= 0.01 and dec[2] == want_lsq[1]
    assert abs(db_old - want_ref[0]) <= 0.01 and old[2] == want_ref[1]


QT_KEYS = [(tag, k, bmin, t) for tag, k, bmin in ((3, 1, 4), (6, 1, 4), (6, 8, 8)) for t in (1200.0, 600.0)]


@pytest.mark.parametrize("tag,n_iso,B_min,threshold", QT_KEYS)
def test_quadtree_leaves_bytes_and_psnr_lena(lena_colored, lena_argb, lena_lsq, lena_ref, tag, n_iso, B_min, threshold):
    levels = qm.levels(16, B_min)
    for which, cbs in ((0, {B: lena_ref[(B, n_iso)] for B in levels}),
                       (1, {B: (lena_lsq[(B, n_iso)]["qrows"], lena_lsq[(B, n_iso)]["iso"]) for B in levels})):
        if tag == 3:
            leaves = qr.encode(lena_argb, W, H, 16, B_min, 0, threshold, {B: q for B, (q, _) in cbs.items()})
            run = qr.write_run(leaves, W, H, 16, B_min, 0)
            img = qr.decode(run)[0]
        else:
            leaves = im.encode(lena_argb, W, H, 16, B_min, 0, n_iso, threshold, cbs)
            run = im.write_qt(leaves, W, H, 16, B_min, 0)
            img = im.decode_qt(run)[0]
        db = 10.0 * np.log10(255.0 ** 2 / np.mean((img.astype(np.float64) - lena_colored) ** 2))
        print(f"tag {tag} n_iso={n_iso} 16 -> {B_min} threshold={threshold} {('reference', 'least squares')[which]}: {len(leaves)} leaves, {len(run)} B, {db:.3f} dB")
        want = QT[(tag, n_iso, B_min, threshold)][which]
        assert (len(leaves), len(run)) == want[:2] and abs(db - want[2]) <= 0.01


def test_refusals_without_a_device(lena_argb):
    from fic_amd import capi
    L = capi.lib()
    a = np.ascontiguousarray(lena_argb[:64 * 64], np.int32)
    nr = 256
    i32 = lambda n: np.zeros(n, np.int32)
    f32 = lambda: np.zeros(nr, np.float32)
    idx, aa, bR, bG, bB, iso, q, E = i32(nr), f32(), f32(), f32(), f32(), i32(nr), i32(5 * nr), np.zeros(nr, np.int64)
    p = capi.ptr

    def one_shot(argb, n_iso):
        return L.fic_encode_rgb_lsq_argb(p(argb, C.c_int32) if argb is not None else None, 64, 64, 4, 29, n_iso, 0, p(idx, C.c_int32),
                                         p(aa, C.c_float), p(bR, C.c_float), p(bG, C.c_float), p(bB, C.c_float), p(iso, C.c_int32),
                                         p(q, C.c_int32), None, p(E, C.c_int64))

    assert one_shot(a, 3) == -3 and "1 or 8 isometries" in capi.last_error()
    assert one_shot(None, 1) == -3
    leaves, n = i32(9 * 256), C.c_int()
    nan = float("nan")
    assert L.fic_encode_rgb_quadtree_lsq_argb(None, 64, 64, 16, 4, 0, 600.0, 0, p(leaves, C.c_int32), 256, C.byref(n)) == -3
    assert L.fic_encode_rgb_quadtree_lsq_argb(p(a, C.c_int32), 64, 64, 16, 4, 0, nan, 0, p(leaves, C.c_int32), 256, C.byref(n)) == -3
    assert "NaN" in capi.last_error()
    assert L.fic_encode_rgb_quadtree_iso_lsq_argb(None, 64, 64, 16, 4, 0, 8, 600.0, 0, p(leaves, C.c_int32), 256, C.byref(n)) == -3
    assert L.fic_encode_rgb_quadtree_iso_lsq_argb(p(a, C.c_int32), 64, 64, 16, 4, 0, 8, nan, 0, p(leaves, C.c_int32), 256, C.byref(n)) == -3
    assert L.fic_encode_rgb_quadtree_iso_lsq_argb(p(a, C.c_int32), 64, 64, 16, 4, 0, 3, 600.0, 0, p(leaves, C.c_int32), 256, C.byref(n)) != 0
    assert L.fic_rgb_ctx_get_lsq_error_host(None, p(E, C.c_int64)) == -3
    with pytest.raises(capi.FicError):
        capi.search_id("least")
    assert b"0.5" in L.fic_version()
