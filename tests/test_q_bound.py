"""The prune bound of the default sweep k_sweep_q (header of fic_q.hip), checked on the reference model tests/qmodel.py in
the f32 / f64 / f16 arithmetic the kernels use.  No GPU and no HIP library needed; tests/test_gpu_q_bound.py shows that the
model's operands ARE the device's, bit for bit, so these are statements about the sweep's real operands.

  * |acc - q| + allowance <= E_r on random, extreme and adversarial blocks, plain and folded, B = 4 / 8 / 16; the adversarial
    inputs must come close to the bound (an asserted floor of |acc - q| / E_r), or the check says nothing;
  * the lemmas the derivation rests on: the chunk-start rule, the theta invariant (folded maximum included), operands never
    subnormal, FIC_Q_TAU_ALL above every test value;
  * the tight inputs (qmodel.tight_image) really are tight: many range blocks have a pair X in an earlier domain tile whose
    test value exceeds the exact winner's by more than 2 s E_r -- what the GPU tests need to catch a bound shrunk by s;
  * the same for joint RGB (k_sweep_q<NK, 3>, E_r scaled by the pool-wide Amax) on qmodel.tight_rgb_image."""
import numpy as np
import pytest

import qmodel as M

F32 = np.float32


def _blocks(rng, B, kind, count):
    n = B * B
    if kind == "random":
        return rng.integers(0, 256, (count, n))
    if kind == "halves":                       # 0 / 255 halves: the largest variance
        b = np.zeros((count, n), np.int64)
        for i in range(count):
            b[i, rng.permutation(n)[:n // 2]] = 255
        return b
    if kind == "var1":                         # var = 1 (one pixel one level above a flat block)
        b = np.full((count, n), 77, np.int64)
        b[np.arange(count), rng.integers(0, n, count)] += 1
        return b
    if kind == "spike":                        # single spikes of every height
        b = np.full((count, n), 10, np.int64)
        b[np.arange(count), rng.integers(0, n, count)] = rng.integers(11, 256, count)
        return b
    if kind == "rem0":                         # sums divisible by n (rem = 0)
        b = rng.integers(0, 250, (count, n))
        b[:, 0] += (-b.sum(1)) % n
        return b
    raise ValueError(kind)


def _check_bound(dpix, rpix, B, folded):
    """max (|acc - q| + allowance) / E_r over all pairs of the given domain and range blocks (folded: the even and the odd
    part's errors summed, which bounds the error of |even| + |odd| against max(|q_k|, |q_k'|))."""
    n_iso = 8 if folded else 1
    A = M.domain_operands(dpix, B, folded)
    cols = M.range_columns(rpix, B, n_iso)
    E = np.repeat(M.range_stats(rpix, B)["E_lo"].astype(np.float64), 4 if folded else 1)
    q = M.q_exact(dpix, cols, B, folded)
    if folded:
        h = B * B // 2
        qe = M.q_exact(dpix, np.concatenate([cols[:, :h], 0 * cols[:, h:]], 1), B, True)
        err = np.abs(M.acc_exact(A[:, :h], cols[:, :h]) - qe) + np.abs(M.acc_exact(A[:, h:], cols[:, h:]) - (q - qe))
    else:
        err = np.abs(M.acc_exact(A, cols) - q)
    err = err + M.allowance(A, cols, B * B // 16)
    return (err / E[None, :]).max()


@pytest.mark.parametrize("B", [4, 8, 16])
@pytest.mark.parametrize("folded", [False, True])
def test_bound_on_random_and_extreme_blocks(B, folded):
    if folded and B == 4:
        pytest.skip("B = 4 has no folded mode (8 isometries run as 8 plain columns)")
    rng = np.random.default_rng(100 + B + folded)
    worst = 0.0
    for dk in ("random", "halves", "var1", "spike", "rem0"):
        for rk in ("random", "halves", "var1", "spike", "rem0"):
            worst = max(worst, _check_bound(_blocks(rng, B, dk, 24), _blocks(rng, B, rk, 24), B, folded))
    assert worst <= 1.0, worst


@pytest.mark.parametrize("B,n_iso", sorted(M.TIGHT_SHAPES))
def test_bound_holds_and_is_approached_on_the_tight_inputs(B, n_iso):
    """The structured inputs (two spikes per block: two or three distinct normalised values, every one rounded to f16 the same
    way) come within a stated share of E_r -- a naive search stays near 0.1 -- and never beyond it."""
    g, r0 = M.tight_image(B, n_iso)
    T = M.sweep_tables(g, B, n_iso)
    rp = M.range_pixels(g, B)[r0:]
    dpix = T["pix"]
    folded = T["folded"]
    # the domain blocks that hold a probe pair (all the others are flat or single-spike)
    sel = np.nonzero((dpix != dpix[:, :1]).sum(1) >= 2)[0][:400]
    ratio = _check_bound(dpix[sel], rp[::max(1, len(rp) // 128)], B, folded)
    assert ratio <= 1.0, ratio
    floor = {4: 0.3, 8: 0.3, 16: 0.2}[B]
    assert ratio >= floor, f"tight inputs reach only {ratio:.3f} of E_r (floor {floor})"


def test_model_pool_is_the_oracle_pool(oracle):
    """The model's scale + pool (k_scale / createCodebuch) equals the oracle's, on a ragged and a square image."""
    for (w, h), B in (((200, 200), 4), ((96, 64), 8), ((128, 128), 16)):
        g = np.random.default_rng(w + B).integers(0, 256, (h, w)).astype(np.uint8)
        pix, mean, _ = oracle.pool(oracle.gray_to_argb(g), w, h, B)
        mine = M.pool_pixels(g, B)
        assert (mine == pix).all()
        assert (M.domain_stats(mine, B)["dM"] == mean).all()


def test_chunk_start_rule():
    """A pair X with L_X >= fl(0.26 rem) prunes, in ANY index order, every pair Y with L_Y <= (1 - 2^-18) L_X: exact_error(Y) >
    exact_error(X) strictly, through the f64 quotient, its f32 rounding, r^2 and rem^2 (1 - r^2) in f32.  Every rem of grey
    blocks (1..n-1) and of RGB (up to 3(n-1)), L_X from the threshold up to far beyond rem (|r| > 1: rem is the reference's
    remainder, not a variance)."""
    rems = np.arange(1, 3 * 255 + 1)
    t = np.concatenate([np.geomspace(1.0, 4096.0, 1500), 1.0 + np.linspace(-1e-4, 1e-4, 201)])
    for rem in rems:
        remf = F32(rem)
        lmin = float(F32(M.LMIN * remf))
        LX = np.concatenate([[lmin, np.nextafter(lmin, np.inf)], lmin * t])
        LY = LX * (1.0 - 2.0 ** -18)
        # exact_error from (cov, rem, s64) with s64 = 1: the quotient cov / (rem * s64) is L / rem
        eX = M.exact_error(LX, np.full(LX.shape, rem), np.ones(LX.shape))
        eY = M.exact_error(LY, np.full(LY.shape, rem), np.ones(LY.shape))
        bad = np.nonzero(~(eY > eX))[0]
        assert bad.size == 0, (rem, LX[bad[0]], eX[bad[0]], eY[bad[0]])


def test_theta_invariant():
    """theta = fl(fl((m - E)(1 - 2^-17)) - E) satisfies theta + E <= (1 - 2^-18) L(X) for every L(X) >= m - E -- checked at the
    worst L(X) = m - E, in f64 on the f32 values, for m and E over their whole range; and for the folded maximum, where m
    is the f32 sum fl(|Be| + |Bo|) of two f32 values (rounded up by up to half an ulp).  Only theta >= 0 matters: a negative
    theta flags every pair."""
    rng = np.random.default_rng(7)
    E = F32(np.concatenate([np.geomspace(1.6e-5, 40.0, 400), [M.EABS]]))
    m = F32(np.geomspace(1e-5, 1.0e5, 3000))
    mm, EE = np.meshgrid(m, E)
    keep = mm - EE > 0
    mm, EE = mm[keep], EE[keep]
    th = M.theta_from_pair(mm, EE)
    # (a negative theta prunes nothing: every test value is >= 0 > theta; there f32 rounding of m - E - E may exceed the slack)
    pos = th >= 0
    assert pos.sum() > len(th) // 2
    assert (th[pos].astype(np.float64) + EE[pos] <= (1 - 2.0 ** -18) * (mm[pos].astype(np.float64) - EE[pos])).all()
    a = F32(rng.uniform(0, 4000, 200000))
    b = F32(rng.uniform(0, 1, 200000) * a)
    Ef = F32(rng.uniform(1.6e-5, 3.0, 200000))
    s = (a + b).astype(F32)                                   # the device's |even| + |odd|
    ok = s.astype(np.float64) - Ef > 0
    th = M.theta_from_pair(s[ok], Ef[ok])
    true_lx = a[ok].astype(np.float64) + b[ok] - Ef[ok]       # max(|q_k|, |q_k'|) >= |Be| + |Bo| - E
    pos = th >= 0
    assert (th[pos].astype(np.float64) + Ef[ok][pos] <= (1 - 2.0 ** -18) * true_lx[pos]).all()


@pytest.mark.parametrize("B", [4, 8, 16])
def test_operands_never_subnormal(B):
    """The smallest non-zero |x| (plain: |d - dM| = 1; folded: |a + b - 2 dM| = 1 or |a - b| = 1, halved) over the largest
    variance a block can have (0 / 255 in every proportion) is a normal f16 (> 2^-14)."""
    n = B * B
    worst = None
    for k in range(1, n):
        blk = np.zeros((1, n), np.int64)
        blk[0, :k] = 255
        blk[0, k] = 1 if k < n - 1 else 0                   # a unit step next to the extremes
        st = M.domain_stats(blk, B)
        w = st["w"][0]
        for v in (F32(1.0) * w, (F32(1.0) * w) * F32(0.5)):
            h = np.float16(v)
            worst = h if worst is None else min(worst, h)
    assert float(worst) > 2.0 ** -14, worst
    # and the model's operands of real blocks: every non-zero element is normal
    rng = np.random.default_rng(B)
    for folded in (False, True):
        A = M.domain_operands(np.concatenate([_blocks(rng, B, k, 64) for k in ("random", "halves", "var1", "spike")]), B, folded)
        nz = np.abs(A[A != 0].astype(np.float64))
        assert nz.min() > 2.0 ** -14


def test_tau_all_is_above_every_test_value():
    """FIC_Q_TAU_ALL ("never flagged") exceeds the largest test value: grey |acc| <= sum |A||B| <= n * 510 (|x| <= 1, folded
    range parts up to 510); joint RGB, where the operand is greyD / vD with vD as small as 1 and |greyR| <= 765: n * 765 * 765."""
    assert float(M.TAU_ALL) > 256 * 510 * 1.0
    assert float(M.TAU_ALL) > 256 * 765 * 765.0


# Floors of the counts measured on the committed generator (qmodel.tight_image, seed 1): at s = 1 / 2 none (the bound is
# sound; halving E_r is not detectable this way), at 1/4 and 1/8 these many range blocks.
WITNESS_FLOOR = {(4, 1): (35, 150), (4, 8): (50, 200), (8, 1): (30, 120), (8, 8): (6, 90), (16, 1): (3, 50), (16, 8): (0, 8)}


@pytest.mark.parametrize("B,n_iso", sorted(M.TIGHT_SHAPES))
def test_tight_inputs_have_prune_witnesses(oracle, B, n_iso):
    """Range blocks of the tight images where a pair X of an earlier domain tile has |acc_X| - |acc_W| >= 2 s E_r (more
    exactly: its theta with E_r shrunk to s E_r reaches the winner W's test value, MFMA allowances included) while W is the
    exact winner (oracle).  A one-chunk sweep whose E_r is s times too small then skips the winner: the images are built for
    s = 1/8 (q_eshift = 3) and most of them hold witnesses at s = 1/4 too.  None at s = 1: the bound holds."""
    g, r0 = M.tight_image(B, n_iso)
    S = g.shape[0]
    G = M.Geom(S, S, B, n_iso)
    ref = oracle.encode_gray(oracle.gray_to_argb(g), S, S, B, G.Dw, n_iso, r0, G.Nr)
    T = M.sweep_tables(g, B, n_iso)
    win, iso = ref["info"][:, 0].astype(np.int64), ref["iso"]
    counts = {s: int(M.prune_witnesses(T, win, iso, s, r0)[0].sum()) for s in (1.0, 0.5, 0.25, 0.125)}
    f4, f8 = WITNESS_FLOOR[(B, n_iso)]
    assert counts[1.0] == 0 and counts[0.5] == 0, counts
    assert counts[0.25] >= f4 and counts[0.125] >= f8, counts


@pytest.mark.parametrize("B", [4, 8, 16])
def test_rgb_bound_with_amax(B):
    """Joint RGB: |acc - kovarianz / vD| + allowance <= E_r, where E_r scales with Amax (the largest rounded-up domain norm of
    the pool) -- against the exact integer kovarianz and against the reference's f32 sequential one (the value it compares),
    on random colour, low-contrast colour (vD small: large operands near Amax) and grey-as-colour images.  The square roots
    are taken one ulp low (the device's are within one ulp).  These inputs reach ~0.1-0.2 of E_r: Amax is a pool-wide
    factor and their winning candidates lie far below it.  The inputs that sit against the colour bound are
    qmodel.tight_rgb_image (the tests below; tests/test_gpu_rgb_q_bound.py shows that a shrunk RGB bound is caught on them)."""
    rng = np.random.default_rng(3 + B)
    imgs = {"random": rng.integers(0, 256, (64, 64, 3)), "lowamp": 120 + rng.integers(-3, 4, (64, 64, 3)),
            "grey": np.repeat(rng.integers(0, 256, (64, 64, 1)), 3, 2)}
    worst = 0.0
    for img in imgs.values():
        rgb = img.astype(np.uint8)
        psum, msum, vD = M.rgb_pool(rgb, B)
        gR, vR = M.rgb_range(rgb, B)
        A, norm = M.rgb_domain_operands(psum, msum, vD, -1)
        E = M.rgb_error_bound(gR, norm.max(), 0, -1).astype(np.float64)
        acc = M.acc_exact(A, gR)
        allow = M.allowance(A, gR, B * B // 16)
        live = vD != 0
        q = ((psum - msum[:, None]) @ gR.T)[live] / vD[live, None].astype(np.float64)
        qJ = M.rgb_kov_java(gR, psum, msum)[live].astype(np.float64) / vD[live, None]
        for qq in (q, qJ):
            worst = max(worst, ((np.abs(acc[live] - qq) + allow[live]) / E[None, :]).max())
    assert worst <= 1.0, worst
    assert worst >= 0.02, worst


# ---------------------------------------------------------------------------------------------------------------------
# joint RGB on the tight colour inputs (qmodel.tight_rgb_image)
# ---------------------------------------------------------------------------------------------------------------------
_RGB_TIGHT = {}


def _rgb_tight(B):
    if B not in _RGB_TIGHT:
        rgb, r0 = M.tight_rgb_image(B)
        _RGB_TIGHT[B] = (rgb, r0, M.rgb_sweep_tables(rgb, B))
    return _RGB_TIGHT[B]


# Floors of max (|acc - q| + allowance) / E_r on the tight colour inputs, seed 1: measured 0.429 / 0.353 / 0.538 (the same
# against the exact kovarianz and against the f32 sequential one: two spikes per block keep every partial sum below 2^24),
# set at about 60 %.  (2^-11 * 1.07 / 7.0e-4 = 0.75 is the most any input can reach.)
RGB_TIGHT_FLOOR = {4: 0.25, 8: 0.21, 16: 0.32}


@pytest.mark.parametrize("B", [4, 8, 16])
def test_rgb_bound_holds_and_is_approached_on_the_tight_inputs(B):
    """|acc - kovarianz / vD| + allowance <= E_r over every non-flat domain block and every range block of the tight colour
    image, against the exact integer kovarianz and against the reference's f32 sequential one; the worst pair comes within
    a stated share of E_r (random colour images: 0.1-0.2); and the construction holds what it promises: Amax is the norm of
    the blocks with a whole probe pair, which all have the same small vD and norms within 2 % of each other."""
    rgb, r0, T = _rgb_tight(B)
    vD, norm = T["vD"], T["norm"]
    live = vD != 0
    n = B * B
    vd_pair = sum(c % n for c in M.TIGHT_RGB_SHAPES[B][2])
    pair = vD == vd_pair
    assert pair.sum() >= 100 and vD[live].min() == vd_pair
    assert norm[pair].max() == T["amax"] and norm[pair].min() >= 0.98 * float(T["amax"])
    assert not (live & ~pair).any() or norm[live & ~pair].max() < 0.6 * float(T["amax"])
    E = T["rs"]["E"].astype(np.float64)
    acc = M.acc_exact(T["A"], T["gR"].astype(np.float16))
    q = ((T["psum"] - T["msum"][:, None]) @ T["gR"].T)[live] / vD[live, None].astype(np.float64)
    qJ = M.rgb_kov_java(T["gR"], T["psum"][live], T["msum"][live]).astype(np.float64) / vD[live, None]
    for name, qq in (("exact", q), ("java", qJ)):
        worst = ((np.abs(acc[live] - qq) + T["allow"][live]) / E[None, :]).max()
        print(f"[rgb tight] B={B} {name}: worst {worst:.4f}")
        assert worst <= 1.0, (name, worst)
        assert worst >= RGB_TIGHT_FLOOR[B], f"tight colour inputs reach only {worst:.3f} of E_r ({name})"


def test_rgb_model_pool_is_the_oracle_pool(oracle):
    """rgb_pool / rgb_range are the oracle's colour pool and range statistics on the tight colour images: pool pixels, the
    channel means and vD (sum of greyD as the reference accumulates it), greyR and vR."""
    for B in (4, 8, 16):
        rgb, r0, T = _rgb_tight(B)
        S = rgb.shape[0]
        pix, means, vD = oracle.pool_rgb(oracle.rgb_to_argb(rgb), S, S, B)
        assert (pix.sum(2) == T["psum"]).all(), B
        assert (means.sum(1) == T["msum"]).all(), B
        assert (vD == T["vD"]).all(), B
        gR, vR = oracle.range_rgb(oracle.rgb_to_argb(rgb), S, S, B)
        assert (gR == T["gR"]).all() and (vR == T["rs"]["rem"]).all(), B


# Floors of the witness counts on the committed generator (qmodel.tight_rgb_image, seed 1), probe ranges only: none at s = 1
# and 1/2 (the bound is sound); measured at s = 1/4: 511 of 512 / 512 of 512 / 246 of 256 range blocks -- every block size
# reaches the largest detectable shrink, q_eshift = 2 -- and at s = 1/8: 511 / 512 / 256.  Floors at about 60 %.
RGB_WITNESS_FLOOR = {4: (300, 300), 8: (300, 300), 16: (150, 150)}


@pytest.mark.parametrize("B", [4, 8, 16])
def test_rgb_tight_inputs_have_prune_witnesses(oracle, B):
    """Probe ranges of the tight colour image where a pair X of an earlier domain tile reaches, with E_r shrunk to s E_r, a
    theta above the test value of the exact winner W (the oracle's encodeRGB, full search; MFMA allowances included): a
    one-chunk k_sweep_q<NK, 3> whose E_r is s times too small skips W."""
    rgb, r0, T = _rgb_tight(B)
    S = rgb.shape[0]
    ref = oracle.encode_rgb(oracle.rgb_to_argb(rgb), S, S, B, T["G"].Dw)
    win = ref[:, 0].astype(np.int64)
    counts = {s: int(M.rgb_prune_witnesses(T, win, s, r0)[0].sum()) for s in (1.0, 0.5, 0.25, 0.125, 0.0625)}
    print(f"[rgb witnesses] B={B}: {counts}")
    f4, f8 = RGB_WITNESS_FLOOR[B]
    assert counts[1.0] == 0 and counts[0.5] == 0, counts
    assert counts[0.25] >= f4 and counts[0.125] >= f8, counts
    assert counts[2.0 ** -M.TIGHT_RGB_ESHIFT[B]] >= 1 and all(counts[2.0 ** -k] == 0 for k in range(M.TIGHT_RGB_ESHIFT[B]))
