// lsq_rgb_fit_test.cpp -- stand-alone host check of lsq_fit_rgb (csrc/fic_lsq_rgb_fit.h), the fit
// every kernel of the joint-RGB least-squares search calls: on random pairs of blocks its qa, t and E against the definition in
// plain 64-bit integers (mathematical floor) and E against the direct sum over the pixels.  The cases cover V == 0, clamped qa
// on both sides, negative numerators that are no multiple of the divisor (floor against truncation) and negative t in every
// channel, and blocks of 0 and 255 only ("halves"), where at n = 256 V passes 2^31 and C passes 2^31 on either side: the values
// the 64-bit C and the unsigned 32-bit V of the B = 16 route exist for.  Built by tests/test_rgb_lsq_model.py with the host compiler and its sanitizers; never runs on a GPU.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../fractal-image-compression_amd/csrc/fic_lsq_rgb_fit.h"

static long long floordiv(long long a, long long b)   // b > 0
{
    long long q = a / b;
    if (a % b != 0 && a < 0) q -= 1;
    return q;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}

int main()
{
    long long failures = 0, pairs = 0, n_v0 = 0, n_hi = 0, n_lo = 0, n_negnum = 0, n_negt[3] = {0, 0, 0};
    long long n_bigv = 0, n_bigc = 0, n_negbigc = 0;
    static uint8_t r[3][256], d[3][256];
    for (int lgn = 4; lgn <= 8; lgn += 2) {
        const int n = 1 << lgn;
        for (int it = 0; it < 7200; it++) {
            const int kind = it < 6000 ? it % 6 : 6;
            // halves: d is 0 or 255 per pixel, the same in the three channels in every other case; r is d with one pixel in 16
            // flipped, 255 - d with such flips (inverted: a quarter of the cases), independent of d, or d itself
            const int equal = it & 1, mode = (it >> 1) & 3;
            for (int ch = 0; ch < 3; ch++) {
                const uint8_t flat = (uint8_t)rnd();
                for (int i = 0; i < n; i++) {
                    uint8_t dv = (uint8_t)rnd(), rv = (uint8_t)rnd();
                    if (kind == 6) {
                        dv = (equal && ch > 0) ? d[0][i] : ((rnd() & 1) ? 255 : 0);
                        const bool flip = mode < 2 && rnd() % 16 == 0;
                        rv = mode == 2 ? ((rnd() & 1) ? 255 : 0) : (uint8_t)((mode == 1) != flip ? 255 - dv : dv);
                    }
                    if (kind == 1) dv = flat;                                              // flat domain: V == 0 when all three are
                    if (kind == 2) { dv = (uint8_t)(100 + rnd() % 4); rv = (rnd() & 1) ? 255 : 0; }          // low contrast: clamps
                    if (kind == 3) rv = (uint8_t)(255 - dv / 2);                           // negative slope
                    if (kind == 4) rv = (uint8_t)((int)dv * dv / 1020);                    // convex: negative intercepts
                    if (kind == 5) { dv = (uint8_t)(100 + (i & 3)); rv = (i & 3) == (ch == 1 ? 0 : 3) ? 255 : 0; }   // +-clamp by channel mix
                    r[ch][i] = rv;
                    d[ch][i] = dv;
                }
            }
            uint32_t S_r[3], S_d[3], S_rr = 0, S_dd = 0, S_rd = 0;
            long long C = 0, V = 0;
            for (int ch = 0; ch < 3; ch++) {
                long long sr = 0, sd = 0, srd = 0, sdd = 0;
                for (int i = 0; i < n; i++) {
                    sr += r[ch][i]; sd += d[ch][i]; srd += r[ch][i] * d[ch][i]; sdd += d[ch][i] * d[ch][i];
                    S_rr += (uint32_t)r[ch][i] * r[ch][i];
                }
                S_r[ch] = (uint32_t)sr; S_d[ch] = (uint32_t)sd; S_rd += (uint32_t)srd; S_dd += (uint32_t)sdd;
                C += n * srd - sr * sd;
                V += n * sdd - sd * sd;
            }
            if (V >= (1ll << 31)) n_bigv++;
            if (C >= (1ll << 31)) n_bigc++;
            if (C <= -(1ll << 31)) n_negbigc++;
            const LsqRgbFit f = lsq_fit_rgb(lgn, S_r, S_rr, S_d, S_dd, S_rd, C, (uint32_t)V);
            // the definition
            long long qa = 0;
            if (V != 0) {
                qa = floordiv(2000 * C + V, 2 * V);
                if (2000 * C + V < 0 && (2000 * C + V) % (2 * V) != 0) n_negnum++;
                qa = qa < -1000 ? -1000 : (qa > 1000 ? 1000 : qa);
            } else n_v0++;
            if (qa == 1000) n_hi++;
            if (qa == -1000) n_lo++;
            long long t[3], E = 0;
            for (int ch = 0; ch < 3; ch++) {
                const long long m = 2 * (1000ll * S_r[ch] - qa * S_d[ch]);
                t[ch] = ch < 2 ? floordiv(m + 10 * n, 20 * n) : floordiv(m + 1000 * n, 2000 * n);
                if (t[ch] < 0) n_negt[ch]++;
                const long long u = ch < 2 ? 10 * t[ch] : 1000 * t[ch];
                for (int i = 0; i < n; i++) {
                    const long long e = 1000ll * r[ch][i] - qa * d[ch][i] - u;
                    E += e * e;
                }
            }
            pairs++;
            if (f.qa != qa || f.t[0] != t[0] || f.t[1] != t[1] || f.t[2] != t[2] || f.E != E || f.E < 0) {
                if (failures++ < 10)
                    printf("n=%d kind=%d: qa %d / %lld, t {%d %d %d} / {%lld %lld %lld}, E %lld / %lld\n", n, kind, f.qa, qa, f.t[0], f.t[1],
                           f.t[2], t[0], t[1], t[2], f.E, E);
            }
        }
    }
    printf("pairs %lld: V == 0 %lld, qa = 1000 %lld, qa = -1000 %lld, negative numerators off the grid %lld, negative t %lld %lld %lld, "
           "V >= 2^31 %lld, C >= 2^31 %lld, C <= -2^31 %lld\n", pairs, n_v0, n_hi, n_lo, n_negnum, n_negt[0], n_negt[1], n_negt[2], n_bigv,
           n_bigc, n_negbigc);
    if (n_v0 < 100 || n_hi < 100 || n_lo < 100 || n_negnum < 100 || n_negt[0] < 100 || n_negt[1] < 100 || n_negt[2] < 100 || n_bigv < 100 ||
        n_bigc < 100 || n_negbigc < 100) {
        printf("a case is not covered\n");
        failures++;
    }
    printf("%lld failures\n", failures);
    return failures ? 1 : 0;
}
