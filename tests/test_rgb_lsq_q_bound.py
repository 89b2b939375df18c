"""The prune bound of the matrix-core joint-RGB least-squares sweep (k_sweep_lsq_rgb_q, fic_lsq_rgb_q.hip, DESIGN.md section
4.22) on the CPU, from the numpy restatement tests/rgblsqqmodel.py: the rounding allowance Er covers the f16 operand error plus the
MFMA's accumulation term in exact rationals, subnormals kept and flushed; theta + Er stays below sqrt(T / n) in exact arithmetic
over the domain of the float chain; the second stage's li at B = 16 magnitudes; the model sweep gives the codebook of
tests/rgblsqmodel.py on every geometry of the GPU file; the tight images of tests/rgblsqqtight.py are what they claim, with the
tables the GPU test imports derived here from the model alone; and the chunk arithmetic under the sanitizers.  No GPU."""
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geomcases as gc  # noqa: E402
import lsqtight as lt  # noqa: E402
import qmodel  # noqa: E402
import rgblsqmodel as lm  # noqa: E402
import rgblsqqmodel as qm  # noqa: E402
import rgblsqqtight as qt  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(B, n_iso) for B in (4, 8, 16) for n_iso in (1, 8)]
IDS = [f"B{B}-iso{n_iso}" for B, n_iso in CASES]
I64 = np.int64


def sample_blocks(B, rng, lena):
    """int64 [*, n, 3]: the design blocks of a tight multi-level image, random blocks (full range, narrow bands, few levels), blocks
    of LenaColored, 0 / 255 blocks (the largest V), and the extremes: flat (V = 0), one pixel of one channel one level off a flat
    block (the smallest V > 0), 0 / 255 halves with one pixel next to its channel's mean (the smallest non-zero |x_i|: subnormal
    in f16)."""
    n = B * B
    img, table = qt.tight_multilevel(B, 1)
    pool = lt._pool(img, B, True)
    tight = pool[sorted({p["g2"] for p in table})[:12]]
    out = [tight, rng.randint(0, 256, size=(24, n, 3)), rng.randint(100, 110, size=(6, n, 3)), rng.choice([0, 3, 250, 255], size=(10, n, 3)),
           rng.choice([0, 255], size=(10, n, 3))]
    y, x = rng.randint(0, 256 - B, size=(2, 16))
    out.append(np.stack([lena[a:a + B, b:b + B].reshape(n, 3) for a, b in zip(y, x)]))
    flat = np.zeros((3, n, 3), I64)
    flat[1], flat[2] = (77, 130, 9), 255
    one = np.zeros((2, n, 3), I64)
    one[0, 0, 1], one[1], one[1, 3, 2] = 1, 255, 254
    half = np.where(np.arange(n) < n // 2, 0, 255)
    halves = np.stack([np.stack([half, half[::-1], np.where(np.arange(n) % 2, 255, 0)], axis=1),
                       np.stack([half, half, half], axis=1)])
    near = np.stack([halves[1].copy() for _ in range(4)])
    for i, v in enumerate((127, 128, 126, 135)):
        near[i, i, i % 3] = v
    # n d_0 - S_d = 1, 2, 3, 5 in channel 0: pixel 0 at v, pixel 1 at w = (n - 1) v - 255 n / 2 - that, the others 0 / 255 in halves
    v = -(-(255 * n // 2 + 6) // (n - 1))
    tiny = np.stack([halves[1].copy() for _ in range(4)])
    for i, t in enumerate((1, 2, 3, 5)):
        tiny[i, 0, 0], tiny[i, 1, 0] = v, (n - 1) * v - 255 * n // 2 - t
        assert 0 <= tiny[i, 1, 0] <= 255 and n * tiny[i, 0, 0] - tiny[i, :, 0].sum() == t
    return np.concatenate([np.asarray(b, I64) for b in out + [flat, one, halves, near, tiny]])


def le_root(a, N, c):
    """a * sqrt(N) <= c for rationals a, c and an integer N > 0, exactly."""
    if a <= 0:
        return c >= 0 or a * a * N >= c * c
    return c >= 0 and a * a * N <= c * c


@pytest.mark.parametrize("B", [4, 8, 16])
def test_allowance_covers_the_operand_error_in_exact_rationals(B, lena_colored):
    """|acc_model - q| + the accumulation term <= Er for every (pool block, range block, isometry) of the sample: acc_model the
    exact dot product of the f16 operands (integers over 2^24), q = C / sqrt(n V) compared through squares, the accumulation term
    2^-24 * 17 NK * sum |A||B| (fic_q.hip's header), Er from the root 1 ulp LOW; the same with every f16 subnormal of the A rows
    flushed to zero.  float64 over the whole sample first (it also finds the worst pairs), then Fractions on a subsample that
    includes the worst."""
    rng = np.random.RandomState(B)
    d = sample_blocks(B, rng, lena_colored)
    r = sample_blocks(B, rng, lena_colored)
    n, NK, NI = B * B, 3 * B * B // 16, 2
    S, _, V, _ = qm.pool_stats(d)
    assert V.min() == 0 and V[V > 0].min() == n - 1 and V.max() == 3 * n * n * 255 * 255 // 4
    assert (V.max() > 2 ** 31) == (B == 16)
    A = qm.a_rows(d, B)
    assert (A[V == 0] == 0).all() and np.isfinite(A.astype(np.float64)).all()
    norm = np.sqrt((A.astype(np.float64) ** 2).sum(1))
    assert np.abs(norm[V > 0] - 1.0).max() < 2.0 ** -10          # the exact row has unit 2-norm over the 3 n entries
    xs = qm.planar(n * d - S[:, None, :]).reshape(-1, 3, n).sum(2)
    assert (xs == 0).all()                                        # and sums to zero per channel
    sub = (A != 0) & (np.abs(A.astype(np.float64)) < 2.0 ** -14)
    if B >= 8:
        assert sub.sum() >= 3, "the sample has no f16 subnormal operand"
    Bc = qm.b_columns(r, B, NI)
    assert np.abs(Bc).max() <= 255 and (Bc.astype(np.float16).astype(I64) == Bc).all()
    st = qm.range_stats(r, B)
    assert (st["Er3"][0] <= st["Er3"][1]).all() and (st["Er3"][1] <= st["Er3"][2]).all()
    Er_low = np.repeat(st["Er3"][0], NI)
    q = qm.q_exact(d, Bc, B)
    # the exact integer C of the definition, whatever the three m_r are
    cp = qm.planar(qm.copies(r, B, NI).reshape(-1, n, 3))
    C = n * (qm.planar(d) @ cp.T) - (S[:, None, :] * np.repeat(st["S_r"], NI, axis=0)[None, :, :]).sum(2)
    assert (C == qm.planar(n * d - S[:, None, :]) @ Bc.T).all()
    worst, checked = 0.0, 0
    for rows in (A, qm.flushed(A)):
        err = np.abs(qmodel.acc_exact(rows, Bc) - q) + qmodel.allowance(rows, Bc, NK)
        ratio = err / Er_low[None, :].astype(np.float64)
        assert (ratio <= 1.0).all(), float(ratio.max())
        worst = max(worst, float(ratio.max()))
        # exact: A * 2^24 are integers
        AI = np.rint(rows.astype(np.float64) * 2.0 ** 24).astype(I64)
        assert (AI.astype(np.float64) * 2.0 ** -24 == rows.astype(np.float64)).all()
        accI, absI = AI @ Bc.T, np.abs(AI) @ np.abs(Bc).T
        order = np.argsort(ratio, axis=None)[::-1]
        pick = np.concatenate([order[:300], order[rng.randint(300, order.size, 900)]])
        for flat_i in pick.tolist():
            i, j = divmod(flat_i, Bc.shape[0])
            acc = Fraction(int(accI[i, j]), 2 ** 24)
            m = Fraction(float(Er_low[j])) - Fraction(17 * NK * int(absI[i, j]), 2 ** 48)
            assert m > 0
            if V[i] == 0:
                assert acc == 0 and C[i, j] == 0
            else:
                N, c = n * int(V[i]), int(C[i, j])
                assert le_root(acc - m, N, c) and le_root(-(acc + m), N, -c)      # acc - m <= q <= acc + m
            checked += 1
    print(f"B={B}: largest (|acc - q| + accumulation) / Er = {worst:.3f}, {int(sub.sum())} subnormal operands, {checked} pairs in exact rationals")
    assert worst > 0.05 and checked >= 2000                       # the sample does reach into the allowance


@pytest.mark.parametrize("B", [4, 8, 16])
def test_theta_plus_er_stays_below_the_bound(B):
    """theta + Er < sqrt(T / n) = sqrt(Ti) / (1000 B) wherever Ti > 0, in exact rationals, for the three candidates of each root:
    Ti log-uniform, uniform, perfect squares and their neighbours, the corners (10^6 R up to 2^51.6 at B = 16); Er from ss over
    its whole range."""
    n = B * B
    R_max = 3 * n * n * 255 * 255 // 4
    T_max = 10 ** 6 * R_max
    assert T_max < 2 ** 52 and (R_max > 2 ** 31) == (B == 16)
    rng = np.random.RandomState(40 + B)
    N = 5000

    def spread(top):
        return np.minimum(np.exp(rng.uniform(0, np.log(top), N)).astype(I64), top)

    def squares(top):
        m = np.minimum(np.sqrt(spread(top).astype(np.float64)).astype(I64) + 1, int(np.sqrt(top)))
        return np.clip(m * m + rng.randint(-1, 2, N), 0, top)

    corners = np.array([0, 1, 2, 3, 4, T_max - 1, T_max], I64)
    Ti = np.concatenate([spread(T_max), rng.randint(0, T_max + 1, N, dtype=I64), squares(T_max), np.repeat(corners, 40)])
    ss_max = 3 * n * (255 * 255 + 1) // 4
    assert ss_max < 2 ** 24
    ss = np.concatenate([spread(ss_max), rng.randint(0, ss_max + 1, N), squares(ss_max), np.tile(np.array([0, 1, ss_max]), 94)[:corners.size * 40]])
    assert Ti.size == ss.size
    checked = 0
    for eu in (-1, 0, 1):
        Er = qm.allowance_er(ss, B, 0, eu)
        for tu in (-1, 0, 1):
            th = qm.theta(Ti, Er, B, 0, tu)
            for t, e, ti in zip(th.tolist(), Er.tolist(), Ti.tolist()):
                s = Fraction(t) + Fraction(e)
                if ti > 0:
                    assert s < 0 or s * s * (10 ** 6 * n) < ti, (ti, t, e)
                    assert t >= 0 or s * s * (10 ** 6 * n) < ti   # also where a < Er and the difference is negative
                    checked += 1
                else:
                    assert t < 0                                  # Ti = 0: theta = -Er, everything is flagged
    assert checked >= 9 * 3 * N
    # without the safety factor the chain is NOT below the bound everywhere (Er = 0): the factor is needed, the samples can tell
    raw = qm.theta(Ti, np.zeros(Ti.size, np.float32), B, 0, 0, safety=1.0)
    over = sum(1 for t, ti in zip(raw.tolist(), Ti.tolist()) if Fraction(t) ** 2 * (10 ** 6 * n) > ti)
    assert over >= 20
    # ... and a factor on the other side of one, 1 + 2^-18, is above it nearly everywhere
    up = qm.theta(Ti[Ti > 2 ** 20], np.zeros(int((Ti > 2 ** 20).sum()), np.float32), B, 0, 0, safety=1.0 + 2.0 ** -18)
    assert all(Fraction(t) ** 2 * (10 ** 6 * n) > ti for t, ti in zip(up.tolist(), Ti[Ti > 2 ** 20].tolist()))
    # the widening of "lsq_tau_widen" puts theta + Er above the bound for large Ti
    wide = qm.theta(np.full(4, T_max), np.zeros(4, np.float32), B, 17)
    assert all(Fraction(t) ** 2 * (10 ** 6 * n) > T_max for t in wide.tolist())


def test_second_stage_bound_at_b16_magnitudes():
    """li^2 * 10^6 < Ti * V' for Ti > 0, V' > 0 up to the corners V, R = 3 n^2 255^2 / 4 = 2^31.57 of B = 16: li passes 2^31 there
    (a signed 32-bit li or C is wrong), stays below 2^32, and the int64 comparison |C| <= li is the exact test."""
    n = 256
    top = 3 * n * n * 255 * 255 // 4
    rng = np.random.RandomState(16)
    N = 20000
    V = np.concatenate([rng.randint(1, top + 1, N, dtype=I64), np.full(2000, top), top - rng.randint(0, 1000, 2000), rng.randint(1, 1000, 2000)])
    R = np.concatenate([rng.randint(1, top + 1, N, dtype=I64), top - rng.randint(0, 1000, 2000), np.full(2000, top), rng.randint(1, top + 1, 2000, dtype=I64)])
    E = np.minimum((rng.random_sample(R.size) ** 4 * 10 ** 6 * R / n).astype(I64), 10 ** 6 * R // n)
    Ti = 10 ** 6 * R - n * E
    assert (Ti >= 0).all() and Ti.max() > 2 ** 51
    keep = Ti > 0
    Ti, V = Ti[keep], V[keep]
    li = lt.li_model(Ti, V, rgb=True)
    assert li.max() >= 2 ** 31 and li.max() < 2 ** 32
    for l, t, v in zip(li.tolist(), Ti.tolist(), V.tolist()):
        assert l * l * 10 ** 6 < t * v, (l, t, v)
    # |C| <= sqrt(R V) < 2^32: C needs 33 signed bits; the model's full-range images reach past 2^31 (tests/test_gpu_rgb_lsq_q.py)
    assert top < 2 ** 32 and top > 2 ** 31
    # the widened chain is above the bound at these magnitudes
    wide = lt.li_model(np.full(4, 10 ** 6 * top), np.full(4, top), 17, rgb=True)
    assert all(l * l * 10 ** 6 > 10 ** 6 * top * top for l in wide.tolist())


def test_an_exact_hit_is_final_and_negative_T_flags_everything():
    R = np.array([0, 5000, 10 ** 9, 7])
    Er = np.full(4, 0.5, np.float32)
    assert (qm.theta_update(R, np.zeros(4, I64), Er, 8) == qm.NEVER).all()                 # E_best = 0: never flagged again
    th = qm.theta_update(R, np.array([1, 10 ** 12, 1, 10 ** 9]), Er, 8)
    assert th[0] == -1.0 and th[1] == -1.0 and th[3] == -1.0 and th[2] > 0                 # T < 0: theta = -1


# the geometries of tests/test_gpu_rgb_lsq_q.py
GEOMS = [(8, 8, 4), (16, 16, 4), (32, 32, 8), (32, 32, 16), (64, 64, 4), (144, 144, 8), (64, 64, 16), (160, 160, 16)]


def _images(w, h):
    y, x = np.mgrid[0:h, 0:w]
    rng = np.random.RandomState(1000 * w + h)
    return {"constant": np.full((h, w, 3), (77, 130, 9), np.uint8),
            "random": rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8),
            "ramp": np.stack([x * 255 // max(w - 1, 1), y * 128 // max(h - 1, 1), 255 - (x + y) * 255 // max(w + h - 2, 1)], -1).astype(np.uint8),
            "lena": gc.rgb_image("lena", w, h, 31 + w + h, 0)}


@pytest.mark.parametrize("n_iso", [1, 8])
@pytest.mark.parametrize("w,h,B", GEOMS, ids=[f"{g[0]}x{g[1]}-B{g[2]}" for g in GEOMS])
def test_the_model_sweep_gives_the_models_codebook(oracle, w, h, B, n_iso):
    """The tile-wise sweep with its prune gives rgblsqmodel.encode's winners on every geometry of the GPU file, with the option
    "chunks" at 1, 3 and 5, subnormals kept and flushed; an exact hit ends a range block's search."""
    for name, rgb in _images(w, h).items():
        want = lm.encode(oracle.rgb_to_argb(rgb), w, h, B, None, n_iso)
        nd = lt._pool(rgb, B, True).shape[0]
        ndt = (nd + 31) // 32
        for chunks, flush in ((1, False), (3, False), (5, True)):
            c = min(chunks, ndt)
            got = qm.sweep(rgb, B, n_iso, tiles_per_chunk=(ndt + c - 1) // c, flush=flush)
            assert (got["E"] == want["E"]).all() and (got["idx_local"] == want["idx_local"]).all() and (got["iso"] == want["iso"]).all(), (name, chunks)
            assert 0 < got["exact"] <= got["pairs"]
        if name == "constant":
            got = qm.sweep(rgb, B, n_iso)
            assert (got["c"] == 0).all() and (got["E"] == 0).all() and got["exact"] == want["E"].size * min(32, nd) * n_iso     # the first tile only


def _changed(got, want):
    return np.flatnonzero((got["E"] != want["E"]) | (got["idx_local"] != want["idx_local"]) | (got["iso"] != want["iso"]))


@pytest.mark.parametrize("B,n_iso", CASES, ids=IDS)
def test_probes_are_what_they_claim(oracle, B, n_iso):
    W = qt.SIDE[B]
    n = B * B
    for kind, (img, table) in (("multi-level", qt.tight_multilevel(B, n_iso)), ("two-level", qt.two_level(B, n_iso))):
        assert img.shape == (W, W, 3) and len(table) >= 25 and len({p["j"] for p in table}) == len(table)
        pool = lt._pool(img, B, True)
        Dw = int(round(np.sqrt(pool.shape[0])))
        want = lm.encode(oracle.rgb_to_argb(img), W, W, B, None, n_iso)
        j = np.array([p["j"] for p in table])
        # the planned winner, E = 0 exactly once
        assert (want["idx_local"][j] == [p["g2"] for p in table]).all() and (want["iso"][j] == [p["k"] for p in table]).all()
        assert (want["E"][j] == 0).all() and all(p["E"] == 0 and p["zeros"] == 1 for p in table)
        own = kind == "multi-level" or B == 16                    # built here: the near fit one block row, so an earlier domain tile, ahead
        if own:
            assert (want["qrows"][j, 1] == [1000 * p["qa"] for p in table]).all()
            for p in table:
                d2, d1 = pool[p["g2"]], pool[p["g1"]]
                assert p["g1"] == p["g2"] - 4 * Dw and p["g1"] // 32 < p["g2"] // 32
                assert np.abs(d1 - d2).sum() == 1 and ((d2 <= 14) | (d2 >= 240)).all() and (d2 % 2 == 0).all()
                assert p["C"] * p["C"] == p["R"] * p["V"] and 0 < p["E_near"] <= 10 ** 6
        # the share of Er that |acc - q| is short by on the winners
        r = lt._blocks(img, B)
        g2 = np.array([p["g2"] for p in table])
        A, Bc, st = qm.a_rows(pool[g2], B), qm.b_columns(r[j], B, n_iso), qm.range_stats(r[j], B)
        col = np.arange(len(table)) * n_iso + np.array([p["k"] for p in table])
        acc, q = qmodel.acc_exact(A, Bc)[np.arange(len(table)), col], qm.q_exact(pool[g2], Bc, B)[np.arange(len(table)), col]
        share = (np.abs(acc) - np.abs(q)) / st["Er"]
        print(f"{kind} B={B} n_iso={n_iso}: (|acc| - |q|) / Er on the winners, median {np.median(share):+.3f}, range {share.min():+.3f} .. {share.max():+.3f}")
        assert (np.abs(share) < 0.5).all()
        if kind == "multi-level":                                 # every design block was drawn for it
            assert (share <= -qt.DRAW_SHARE[B] + 1e-9).all()


@pytest.mark.parametrize("B,n_iso", CASES, ids=IDS)
def test_eshift_the_probes_catch(oracle, B, n_iso):
    """Teeth: Er times 2^-k narrows the bound below the derivation; the smallest k at which the model sweep loses the winner of a
    quarter of the probes is ESHIFT_CAUGHT.  A pair counts as skipped only if it stays skipped with the accumulation allowance
    added to |acc| (bias = 1).  Every row that changes is a probe and gets a larger E; k <= 0 changes nothing."""
    img, table = qt.tight_multilevel(B, n_iso)
    W = qt.SIDE[B]
    want = lm.encode(oracle.rgb_to_argb(img), W, W, B, None, n_iso)
    j = np.array([p["j"] for p in table])
    lost = {}
    for k in (-2, 0, 1, 2, 3, 4):
        got = qm.sweep(img, B, n_iso, eshift=k, bias=1.0)
        ch = _changed(got, want)
        assert np.isin(ch, j).all() and (got["E"][ch] > want["E"][ch]).all()
        lost[k] = ch.size
    print(f"B={B} n_iso={n_iso}: probes that lose their winner at lsq_q_eshift -2, 0, 1..4: {[lost[k] for k in (-2, 0, 1, 2, 3, 4)]} of {len(table)}")
    assert lost[-2] == 0 and lost[0] == 0
    caught = [k for k in (1, 2, 3, 4) if lost[k] * 4 >= len(table)]
    assert caught and caught[0] == qt.ESHIFT_CAUGHT[(B, n_iso)] and caught == list(range(caught[0], 5))


@pytest.mark.parametrize("B,n_iso", CASES, ids=IDS)
def test_widening_the_two_level_probes_catch(oracle, B, n_iso):
    """The two-level images under "lsq_tau_widen" = WIDEN_CAUGHT: probes whose near fit is evaluated before their winner (an earlier
    domain tile, or an earlier round of the same tile) lose it; only probes change, and nothing changes without the widening."""
    img, table = qt.two_level(B, n_iso)
    W = qt.SIDE[B]
    want = lm.encode(oracle.rgb_to_argb(img), W, W, B, None, n_iso)
    assert _changed(qm.sweep(img, B, n_iso, bias=1.0), want).size == 0
    got = qm.sweep(img, B, n_iso, widen=qt.WIDEN_CAUGHT[(B, n_iso)], bias=1.0)
    ch = _changed(got, want)
    print(f"B={B} n_iso={n_iso}: {ch.size} of {len(table)} probes change under the widening")
    assert ch.size >= 1 and np.isin(ch, [p["j"] for p in table]).all() and (got["E"][ch] > want["E"][ch]).all()


@pytest.mark.parametrize("n_iso", [1, 8])
def test_the_tie_image_is_what_it_claims(oracle, n_iso):
    """Exact hits of the probe at pool blocks 1, 4, 7, 10 (isometry 0) and nowhere else; 1 and 4 lie in rounds 1 and 0 of the first
    domain tile (rgblsqqmodel.ROUNDS), so the kernel meets the later candidate first; the model sweep gives block 1."""
    img, j = qt.tie_image()
    E = lt.pair_sums(img, 4, n_iso, True, rows=[j])["E"][0]
    assert [tuple(z) for z in np.argwhere(E == 0)] == [(1, 0), (4, 0), (7, 0), (10, 0)]
    rnd = {row: e for e, grp in enumerate(qm.ROUNDS) for row in grp}
    assert rnd[4] < rnd[1]
    want = lm.encode(oracle.rgb_to_argb(img), 32, 32, 4, None, n_iso)
    assert want["idx_local"][j] == 1 and want["iso"][j] == 0 and want["E"][j] == 0
    for tpc in (None, 1):
        got = qm.sweep(img, 4, n_iso, tiles_per_chunk=tpc)
        assert _changed(got, want).size == 0


def test_chunk_arithmetic_under_the_sanitizers(tmp_path):
    """tests/cpp/lsq_q_chunks_test.cpp: fic_lsq_q_chunks.h (what the launchers and the C ABI call) as a program of its own, with
    the host compiler's address and undefined-behaviour sanitizers where it has their runtimes."""
    src = os.path.join(ROOT, "tests", "cpp", "lsq_q_chunks_test.cpp")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    ok = subprocess.run(["g++"] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode == 0
    if not ok or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        san = []
    print("lsq_q_chunks_test built " + ("with " + san[0] if san else "WITHOUT sanitizers (the host compiler has no runtimes for them)"))
    exe = str(tmp_path / "lsq_q_chunks_test")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + san + [src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "lsq_q_chunks.txt")], capture_output=True, text=True)
    assert r.returncode == 0 and "\n0 failures" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr
