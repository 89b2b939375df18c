// fic_lsq_q_tile.h -- what the two matrix-core least-squares sweeps, k_sweep_lsq_q (grey, fic_lsq_q.hip) and
// k_sweep_lsq_rgb_q (joint RGB, fic_lsq_rgb_q.hip, 4.22), and their prep kernels share: the operand fragment packers and the
// epilogue of one 32 x 32 accumulator tile -- the flagged mask (every kernel), the 16 rounds of exact evaluation with theta
// raised from tau (RGB, grey B = 16).  f16_pair / max16_abs are also fic_q.hip's.  Device code, all inlined; the proofs ("Ties",
// "Within a tile", "Exact hit", "Padding") are in the headers of the two .hip files, which keep what differs (evaluators, tau
// chains, Er, the grey LDS queue, the RGB grouped prefetch) and, each its own, the wave decode, the (E, c) publish merge and the
// statistics: those cost sweep time when they came from here (profiles/lsq_q_tile_refactor.json).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "fic_devfn.h"
#include "fic_lsq_fit.h"                       // FIC_LSQ_E_NONE

typedef int v4i __attribute__((ext_vector_type(4)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

#define FIC_LSQ_Q_EABS 1.6e-5f                 // absolute term of the rounding allowance Er
#define FIC_LSQ_Q_NEVER 3.0e38f                // theta "never flagged": padding columns, and range blocks with an exact hit
#define FIC_LSQ_Q_AWAY 1.00000023841857910156f // 1 + 2^-22: a negative theta is rounded away from zero

// two floats -> packed f16 pair (round to nearest even), element 0 in the low half
__device__ __forceinline__ int f16_pair(float lo, float hi)
{
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    h2 v = {(_Float16)lo, (_Float16)hi};
    return __builtin_bit_cast(int, v);
}

// Every node is a three-input maximum (v_max3_f32 with |.| source modifiers): a two-input fmaxf of MFMA results costs two
// extra canonicalising v_max_f32 x, x under IEEE mode, hence the constant 0 as third operand at the root.
__device__ __forceinline__ float max3f(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }
__device__ __forceinline__ float max16_abs(const v16f& a)
{
    const float m0 = max3f(fabsf(a[0]), fabsf(a[1]), fabsf(a[2]));
    const float m1 = max3f(fabsf(a[3]), fabsf(a[4]), fabsf(a[5]));
    const float m2 = max3f(fabsf(a[6]), fabsf(a[7]), fabsf(a[8]));
    const float m3 = max3f(fabsf(a[9]), fabsf(a[10]), fabsf(a[11]));
    const float m4 = max3f(fabsf(a[12]), fabsf(a[13]), fabsf(a[14]));
    return max3f(max3f(m0, m1, m2), max3f(m3, m4, fabsf(a[15])), 0.0f);
}

// ---- prep: one fragment slot = 8 consecutive operand bytes (two little-endian words) as 4 packed f16 pairs -------------------
// Slot (m, lane) of a 32-row (or 32-column) tile holds elements [16 m + 8 (lane >> 5), +8) of row / column lane & 31: the
// v_mfma_f32_32x32x16_f16 shape.
__device__ __forceinline__ int lsq_q_byte(uint32_t w0, uint32_t w1, int u) { return (int)(((u < 4 ? w0 : w1) >> (8 * (u & 3))) & 0xffu); }
// pool row: f16( fl((float)(n px - S) * w) )
__device__ __forceinline__ v4i lsq_q_pack_pool(uint32_t w0, uint32_t w1, int lgn, int S, float w)
{
    v4i v;
#pragma unroll
    for (int u = 0; u < 4; u++)
        v[u] = f16_pair(__fmul_rn((float)((lsq_q_byte(w0, w1, 2 * u) << lgn) - S), w), __fmul_rn((float)((lsq_q_byte(w0, w1, 2 * u + 1) << lgn) - S), w));
    return v;
}
// range column: f16( px - m_r ), an integer in [-255, 255]
__device__ __forceinline__ v4i lsq_q_pack_range(uint32_t w0, uint32_t w1, int mr)
{
    v4i v;
#pragma unroll
    for (int u = 0; u < 4; u++) v[u] = f16_pair((float)(lsq_q_byte(w0, w1, 2 * u) - mr), (float)(lsq_q_byte(w0, w1, 2 * u + 1) - mr));
    return v;
}

// ---- sweep: the epilogue of one 32 x 32 accumulator tile -------------------------------------------------------------------------
// Accumulator element e of lane l: column l & 31, domain row lsq_q_row(e, l >> 5) of the tile.
__device__ __forceinline__ int lsq_q_row(int e, int half) { return (e & 3) + 8 * (e >> 2) + 4 * half; }

// bit e: element e of this lane is flagged (|acc| above theta, or theta < 0), its row is one of the tile's `nreal` real rows
// (>= 1) and the column belongs to a real range block
__device__ __forceinline__ uint32_t lsq_q_flagged(const v16f& acc, float theta, int nreal, int half, bool ok)
{
    uint32_t hm = 0;
#pragma unroll
    for (int e = 0; e < 16; e++) hm |= !(fabsf(acc[e]) <= theta) ? 1u << e : 0u;
    if (nreal < 32) {
#pragma unroll
        for (int e = 0; e < 16; e++)
            if (lsq_q_row(e, half) >= nreal) hm &= ~(1u << e);
    }
    return ok ? hm : 0u;
}

// minimum over the lanes that share a range block: the two lane halves and the 2^CSHIFT adjacent columns
template <int CSHIFT>
__device__ __forceinline__ long long lsq_q_group_min(long long e)
{
    long long o = __shfl_xor(e, 32, 64);
    e = o < e ? o : e;
    if constexpr (CSHIFT == 3) {
#pragma unroll
        for (int off = 1; off <= 4; off <<= 1) {
            o = __shfl_xor(e, off, 64);
            e = o < e ? o : e;
        }
    }
    return e;
}

// theta of the prune test from tau (< 0: T < 0, everything is flagged): fl(tau / B - Er), rounded away from zero where negative
__device__ __forceinline__ float lsq_q_theta(float tau, float invB, float er)
{
    if (tau < 0.0f) return -1.0f;
    const float th = __fsub_rn(__fmul_rn(tau, invB), er);                       // tau / B is exact
    return th < 0.0f ? __fmul_rn(th, FIC_LSQ_Q_AWAY) : th;
}

// The flagged pairs `hm` of one tile (first pool block d0), 16 rounds: round e takes element e of every lane, rows
// lsq_q_row(e, 0) and, in the other lane half, 4 more.  evaluate(d, tl, bE, bC) is the file's exact evaluation under the second
// stage's bound tl; tau_of(E) its tau chain for a smallest error E (-1 where T < 0).  After a round tl is refined from the
// smallest E of the range block so far PLUS ONE ("Within a tile").  Then theta and tau of the column are raised from the
// smallest E over the lanes of the range block ("Ties"); E == 0 ends its search ("Exact hit").
template <int CSHIFT, class Eval, class TauOf>
__device__ __forceinline__ void lsq_q_rounds(uint32_t hm, int d0, int half, bool ok, float er, float invB, float& theta, float& tau, long long& best_E,
                                             uint32_t& best_c, Eval&& evaluate, TauOf&& tau_of)
{
    float tl = tau;
    long long bE = best_E;
    uint32_t bC = best_c;
#pragma unroll 1
    for (int e = 0; e < 16; e++) {
        const bool mine = (hm >> e) & 1u;
        if (__builtin_amdgcn_ballot_w64(mine) == 0) continue;
        if (mine) evaluate(d0 + lsq_q_row(e, half), tl, bE, bC);
        const long long E1 = lsq_q_group_min<CSHIFT>(bE);
        if (E1 != FIC_LSQ_E_NONE) tl = fmaxf(tl, tau_of(E1 + 1));
    }
    best_E = bE;
    best_c = bC;
    const long long Eg = lsq_q_group_min<CSHIFT>(bE);
    if (ok && Eg != FIC_LSQ_E_NONE) {
        if (Eg == 0) {
            theta = FIC_LSQ_Q_NEVER;
        } else {
            tau = tau_of(Eg);
            theta = lsq_q_theta(tau, invB, er);
        }
    }
}
