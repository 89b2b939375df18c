// fic_lsq_fit.h -- the quantised least-squares fit of one (range block, candidate) pair from its exact integer sums (DESIGN.md
// section 4.19; the definitions are in the header of fic_lsq.hip).  Shared by the sweeps of fic_lsq.hip and fic_lsq_q.hip, so
// that every sweep evaluates a pair with the same instructions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#define FIC_LSQ_E_NONE 0x7FFFFFFFFFFFFFFFll

struct LsqFit {
    int qa, qb;
    long long E;
};

// floor(x / 25) for any int x (C's '/' truncates towards zero)
__device__ __forceinline__ int lsq_floordiv25(int x)
{
    const int q = x / 25;
    return q - ((x - q * 25) < 0 ? 1 : 0);
}

// The quantised fit of one pair from its exact sums.  The float quotient qf ~ 100 C / V only proposes qa: two conversions, the
// reciprocal (1 ulp) and two products keep it within 2^-21 relative, so |qf| >= 101 means |100 C / V| > 100.9 and the clamp
// decides; otherwise floor(qf + 1/2) is off by at most one and the remainder of the exact division puts it right -- the result
// is clamp(floor((200 C + V) / (2 V))) exactly.
__device__ __forceinline__ LsqFit lsq_fit(int lgn, int S_r, int S_rr, int S_d, int S_dd, int S_rd, int C, int V)
{
    LsqFit f;
    int qa = 0;
    if (V != 0) {
        const float qf = __fmul_rn(__fmul_rn((float)C, __builtin_amdgcn_rcpf((float)V)), 100.0f);
        if (qf >= 101.0f) qa = 100;
        else if (qf <= -101.0f) qa = -100;
        else {
            qa = (int)floorf(__fadd_rn(qf, 0.5f));
            const long long rem = 200ll * C + V - 2ll * V * qa;    // in [0, 2 V) exactly when qa is the floor
            if (rem < 0) qa -= 1;
            else if (rem >= 2ll * V) qa += 1;
            qa = qa < -100 ? -100 : (qa > 100 ? 100 : qa);
        }
    }
    // |2 (100 S_r - qa S_d) + 100 n| < 2^25; 200 n = 25 * 2^(lgn + 3), and an arithmetic shift is a floor
    const int t = 2 * (100 * S_r - qa * S_d) + (100 << lgn);
    const int qb = lsq_floordiv25(t >> (lgn + 3));
    // E = 10^4 S_rr + qa (qa S_dd + 200 (qb S_d - S_rd)) + 10^4 qb (n qb - 2 S_r);  |qb| <= 766, so the 32-bit factors fit
    const long long inner = (long long)qa * S_dd + 200ll * (qb * S_d - S_rd);
    f.qa = qa;
    f.qb = qb;
    f.E = 10000ll * S_rr + (long long)qa * inner + 10000ll * (qb * (qb * (1 << lgn) - 2 * S_r));
    return f;
}
