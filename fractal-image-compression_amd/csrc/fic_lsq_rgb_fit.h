// fic_lsq_rgb_fit.h -- the quantised fit of one (range block, candidate) pair of the joint-RGB least-squares search (DESIGN.md
// section 4.20) from its exact sums.  Plain C++ without HIP, shared by the kernels of fic_lsq_rgb.hip and by the host check
// tests/cpp/lsq_rgb_fit_test.cpp.
//
// n = B*B = 2^lgn, per channel ch in {R, G, B}: S_r, S_d; summed over the channels: S_rr, S_dd, S_rd.
//   C = sum_ch (n S_rd - S_r S_d)   (|C| <= sqrt(R V) <= 3.2e9 at B = 16: 64 bits),   V = sum_ch (n S_dd - S_d^2) < 2^32
//   qa  = 0 if V == 0 else clamp(floor((2000 C + V) / (2 V)), -1000, 1000)            (1000 C / V to nearest, then the clamp)
//   t_R, t_G = floor((2 (1000 S_r - qa S_d) + 10 n) / (20 n))                         (100 (mean_r - a mean_d) to nearest)
//   t_B      = floor((2 (1000 S_r - qa S_d) + 1000 n) / (2000 n))                     (mean_r - a mean_d to nearest)
//   u = {10 t_R, 10 t_G, 1000 t_B}
//   E = 10^6 S_rr + qa^2 S_dd - 2000 qa S_rd + sum_ch (n u^2 - 2000 u S_r + 2 qa u S_d) = sum_ch sum_i (1000 r - qa d - u_ch)^2
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FIC_HD __host__ __device__ __forceinline__
#else
#define FIC_HD inline
#endif

struct LsqRgbFit {
    int qa, t[3];
    long long E;
};

// floor(x / d) for any int x and d > 0 (C's '/' truncates towards zero)
FIC_HD int lsq_rgb_floordiv(int x, int d)
{
    const int q = x / d;
    return q - ((x - q * d) < 0 ? 1 : 0);
}

// The float quotient qf ~ 1000 C / V only proposes qa: two conversions, a division and a product keep it within 2^-21
// relative, below 10^-3 absolute where |qf| < 1001, so |qf| >= 1001 means |1000 C / V| > 1000.9 and the clamp decides;
// otherwise floor(qf + 1/2) is off by at most one and the remainder of the exact division puts it right -- the result is
// clamp(floor((2000 C + V) / (2 V))) exactly.
FIC_HD LsqRgbFit lsq_fit_rgb(int lgn, const uint32_t S_r[3], uint32_t S_rr, const uint32_t S_d[3], uint32_t S_dd, uint32_t S_rd,
                             long long C, uint32_t V)
{
    LsqRgbFit f;
    int qa = 0;
    if (V != 0) {
        const float qf = ((float)C / (float)V) * 1000.0f;
        if (qf >= 1001.0f) qa = 1000;
        else if (qf <= -1001.0f) qa = -1000;
        else {
            const float fl = qf + 0.5f;
            qa = (int)fl;
            if ((float)qa > fl) qa -= 1;                       // floor of a negative value
            const long long V2 = 2ll * (long long)V;
            const long long rem = 2000ll * C + (long long)V - V2 * qa;    // in [0, 2 V) exactly when qa is the floor
            if (rem < 0) qa -= 1;
            else if (rem >= V2) qa += 1;
            qa = qa < -1000 ? -1000 : (qa > 1000 ? 1000 : qa);
        }
    }
    f.qa = qa;
    // |2 (1000 S_r - qa S_d)| + 1000 n < 2^29 (S_r, S_d <= 255 n <= 65280); 20 n = 5 * 2^(lgn + 2), 2000 n = 125 * 2^(lgn + 4),
    // an arithmetic shift is a floor and floor(floor(x / p) / q) = floor(x / (p q))
    long long e = 1000000ll * (long long)S_rr + (long long)qa * ((long long)qa * (long long)S_dd - 2000ll * (long long)S_rd);
    for (int ch = 0; ch < 3; ch++) {
        const int m = 2 * (1000 * (int)S_r[ch] - qa * (int)S_d[ch]);
        int t, u;
        if (ch < 2) {
            t = lsq_rgb_floordiv((m + (10 << lgn)) >> (lgn + 2), 5);
            u = 10 * t;
        } else {
            t = lsq_rgb_floordiv((m + (1000 << lgn)) >> (lgn + 4), 125);
            u = 1000 * t;
        }
        f.t[ch] = t;
        // |u| <= 5.2e5: n u - 2000 S_r + 2 qa S_d fits 32 bits signed at n <= 256 (1.4e8 + 1.4e8 + 1.4e8)
        e += (long long)u * (long long)(u * (1 << lgn) - 2000 * (int)S_r[ch] + 2 * qa * (int)S_d[ch]);
    }
    f.E = e;
    return f;
}
