// fic_lsq_rgb_q.hip -- the joint-RGB least-squares domain search ("search" = 1 of a colour context, DESIGN.md sections 4.20 and
// 4.22) on the matrix cores, opt-in by the context option "lsq_engine" = 1: k_lsq_rgb_q_prep (operand fragments, per-range
// allowance) and k_sweep_lsq_rgb_q<NK, CSHIFT> (prune GEMM + exact evaluation of the survivors), B = 4 / 8 / 16.  gfx950
// (MI355X / CDNA4) only, wave64.  Compile with -ffp-contract=off.
//
// The matrix core only decides which pairs can be SKIPPED.  Every pair that can win is evaluated by the integer arithmetic of
// fic_lsq_rgb.hip -- S_rd by v_dot4_u32_u8 over the 3 n bytes, C = n S_rd - sum_ch S_r S_d, lsq_fit_rgb (fic_lsq_rgb_fit.h,
// unchanged) -- and the winner is the lexicographic (E, c) minimum, c = pool block * n_iso + isometry; the per-chunk minima go to
// the slots that k_finalize_lsq_rgb merges.  The codebook has the bits of k_sweep_lsq_rgb_fast's / k_sweep_lsq_rgb_generic's.
//
// Operands.  Only the channel sums of S_rr, S_dd, S_rd enter C, V and E, so a block is ONE vector of K = 3 n entries, index
// i = ch * n + pos (pool3[d][ch][pos], rng3's dword ch * DW + pos / 4); NK = 3 n / 16 = 3 / 12 / 48 K-steps of 16.
//     A[d][i] = f16( fl((float)(n d_i - S_d[ch]) * w) ),   w = fl(1 / fl(B * s32)),  s32 = fl32(sqrt((double) V)) as stored
//                                                            (V == 0 or d >= N_d: the row is all zeros)
//     B[i][c] = f16( copy_k[i] - m_r[ch] ),                 m_r[ch] = floor((2 S_r[ch] + n) / (2 n))
// for column c = j * n_iso + k.  The exact row x^[i] = (n d_i - S_d[ch]) / sqrt(n V) has unit 2-norm over the 3 n entries
// (sum_i (n d_i - S_d[ch])^2 = n sum_ch (n S_dd,ch - S_d[ch]^2) = n V) and sums to zero PER CHANNEL (sum_pos (n d - S_d[ch]) =
// n S_d[ch] - n S_d[ch]).  Proof that q is C / sqrt(n V) whatever the three m_r are:
//     q = sum_i x^[i] (copy_k[i] - m_r[ch]) = sum_i x^[i] copy_k[i] - sum_ch m_r[ch] (sum_pos x^[ch, pos]) = sum_i x^[i] copy_k[i]
//       = sum_ch (n S_rd,ch - S_d[ch] S_r[ch]) / sqrt(n V) = C / sqrt(n V).
// The centring only keeps ||b|| small.  B entries are integers in [-255, 255]: exact in f16.  n d_i - S_d[ch] is an integer of
// magnitude <= 255 n <= 65280: exact in f32.
//
// Per range block the prep stores R = sum_ch (n S_rr,ch - S_r[ch]^2) = n S_rr - sum_ch S_r[ch]^2 and Er.  R <= 3 n^2 255^2 / 4
// < 2^31.6 at B = 16: it is stored UNSIGNED (n S_rr itself passes 2^32 there; the difference modulo 2^32 is R, as for V in
// k_lsq_rgb_prep).  ss = sum_i (r_i - m_r[ch])^2 = S_rr - 2 sum_ch m_r S_r + n sum_ch m_r^2 = ||b||^2 is an exact integer:
// per channel sum (r - m_r)^2 = sum (r - mean)^2 + n (mean - m_r)^2 <= n 255^2 / 4 + n / 4, so ss <= 3 n (255^2 + 1) / 4 <
// 768 * 128^2 = 2^23.6 < 2^24 at B = 16, and (float) ss is exact.
//
// The bound.  (4.20) E / 10^6 >= (R - C^2 / V) / n, so a candidate Y cannot beat E_best when C_Y^2 <= T V_Y, T = (10^6 R - n
// E_best) / 10^6 >= 0, i.e. when |q_Y| <= sqrt(T / n) = sqrt(Ti) / (1000 B), Ti = 10^6 R - n E_best an exact int64 (10^6 R <
// 2^51.6, n E < 2^58: no overflow; E < 2^50).  With |acc - q| <= Er it is enough that |acc_Y| <= theta, theta + Er < sqrt(T / n):
//     tau = fl(fl(fl(sqrtf(fl(Ti)) * 0.001f) * (1 - 2^-18)) * widen)      -- k_sweep_lsq_rgb_fast's chain, the same instructions
//     theta = fl( tau * (1/B) - Er )                                      (times 1 + 2^-22 where negative)
// fl(Ti) errs by 2^-24 (2^-25 after the root), the root by at most 1 ulp (2^-23), 0.001f is 0.001 (1 + 2^-24.3), three products
// round by 2^-24 each and the product with the power of two 1/B is exact: together < 2^-21, so the minuend a <= sqrt(T / n) (1 -
// 2^-18)(1 + 2^-21); the subtraction rounds by at most 2^-24 |a - Er| <= 2^-24 a while a >= Er, so theta + Er <= a (1 + 2^-24) <
// sqrt(T / n).  With a < Er the difference is negative; it is multiplied by 1 + 2^-22, which moves it away from zero by more
// than the two roundings can have moved it towards zero: theta <= a - Er (it flags everything anyway).  None of this depends on
// the magnitudes: at B = 16, 10^6 R < 2^51.6 is still an exact int64 and a finite f32, tau < 2^25.8 / 1000.
// theta < 0 flags every pair, zeros included: theta = -1 stands for "nothing evaluated yet" and for T < 0 (then a flat pool block,
// C = V = 0, could still win).  A zero row (V == 0) gives acc == 0 exactly, which passes only theta >= 0, and theta >= 0 implies
// T >= 0: the right condition for such a candidate.
//
// Second stage.  A pair that the GEMM flags has S_rd and C computed exactly and is dropped without the 64-bit fit when |C| <= li,
// li = trunc(fl(tau * s32')) < sqrt(T V') (4.20's proof: the same roundings plus s32' and one product, < 2^-21 against 1 - 2^-18;
// truncation of a non-negative float never rounds up).
//   B <= 8: R, V < 2^27.6, |C| <= sqrt(R V) < 2^31: C is computed modulo 2^32 and read as a signed int, li is an int -- the fast
//           kernel's instructions.
//   B = 16: |C| reaches 3.2e9 and tau * s32' reaches 2^31.6, so neither fits a signed int.  C is computed in 64 bits (n S_rd <
//           2^34 minus lsq_rgb_cross < 2^34: exact) and li = (long long) fl(tau * s32'): the float is < 2^32, its conversion to
//           int64 is exact truncation, and the comparison -li <= C <= li of two exact int64 is |C| <= li < sqrt(T V'): sound with
//           no bound on |C| needed at all.
//
// Rounding allowance.  Er = fl(fl(fl(sqrt(ss)) * c) + abs) * 2^-lsq_q_eshift with
//     c = fl(fl(7.0e-4f + NK * 1.1e-6f) + B * 1.0575e-4f),   abs = 1.6e-5f,
// derived for K = 3 n as follows (all terms relative to ||b|| = sqrt(ss)):
//   * f32 value of x_i: B * s32 exact, s32 twice rounded, a divide and a product: within 2^-22 relative; ||x|| <= 1 + 2^-22.
//   * f16 rounding of a NORMAL entry: 2^-11 relative; sum |dx_i| |b_i| <= 2^-11 ||x|| ||b|| (Cauchy-Schwarz).
//   * a non-zero |x_i| is >= 1 / sqrt(n V) > 2^-20 (V < 2^31.6, n <= 256) and CAN fall below f16's smallest normal 2^-14.  Kept
//     as a subnormal it errs by <= 2^-25; flushed to zero (by the conversion or by the MFMA) it loses |x_i| |b_i| < 2^-14 |b_i|.
//     The allowance relies on neither: per such entry it takes 2^-14 |b_i|, which covers both, and sum |b_i| <= sqrt(3 n) ||b|| =
//     sqrt(3) B ||b||: the term B * 1.0575e-4 (sqrt(3) * 2^-14 = 1.05716e-4).
//   * products of an 8-bit and an 11-bit significand are exact in f32; the accumulation of NK * 16 terms inside the MFMAs adds at
//     most 2^-24 * 17 NK * sum |A||B| (fic_q.hip's header), sum |A||B| <= ||A|| ||b|| <= (1 + 2^-10) ||b||: 1.0143e-6 NK ||b||,
//     the term NK * 1.1e-6 (2^-14.3 ||b|| at NK = 48).
//   Total |acc - q| <= (2^-11 (1 + 2^-10) + 2^-22 + 1.0143e-6 NK + sqrt(3) B 2^-14) ||b|| = (4.8900e-4 + ...) ||b|| against
//   7.0e-4 + 1.1e-6 NK + 1.0575e-4 B: the difference, > 2.1e-4 ||b||, and `abs` cover the roundings of Er itself (five, 2^-24
//   each, and a root 1 ulp low).  ||b|| = 0 means b = 0, acc = 0 = q.  tests/rgblsqqmodel.py restates the prep and
//   tests/test_rgb_lsq_q_bound.py checks |acc - q| + the accumulation term <= Er in exact rationals, subnormals kept and flushed.
//
// Minima.  Colour E is below 2^50, so a 64-bit key (E << 22) | c_rel does not exist.  Each lane keeps its own (E, c) pair, c the
// global candidate in 32 bits, compared lexicographically; the lanes of a range block are merged by xor-shuffles (lane halves,
// and the 8 adjacent columns with 8 isometries).  No atomics, no cap on a chunk's length; the only cap is N_d * n_iso <= 2^32 - 2
// (fic_lsq_q_chunks.h).  The (E, c) order is total, so the merged minimum does not depend on lanes, rounds or chunks.
//
// Survivors.  All three block sizes evaluate the flagged pairs of a tile in its own lanes, in 16 rounds (accumulator element e of
// every lane), the scheme the grey sweep keeps for B = 16: with per-lane minima a queue that hands a pair to ANY lane would need
// a second merge structure in LDS.  The grey sweep's queue (B = 4 / 8) is therefore not used here; where that costs, DESIGN.md
// 4.22 names it.
//
// Ties (4.21's rules).  theta of a range block is only ever derived from E_best over pairs that HAVE been evaluated, all of them
// in domain tiles BEFORE the one under test (or, within a chunk's first tile, nothing: theta = -1).  The candidates of one domain
// tile are tested against the theta of the tiles before it, all flagged pairs of the tile are evaluated, each lane keeps the
// lexicographic (E, c) minimum of what it evaluated, and only then is theta raised from the minimum E over the lanes that share
// the range block.  So a pruned Y has E_Y >= E_best = E_X with c_X < c_Y (X in an earlier tile: a smaller pool index): X wins the
// tie.  No seeding from a tile's largest |acc| and no bound shared between chunks.
// Within a tile.  The rounds are not in the order of c.  Only tau, the second stage's bound, moves between the rounds, and it is
// computed from E_best + 1: a pair Y dropped by it has E_Y >= E_X + 1 > E_X for an evaluated X, so X beats Y in any index order.
// The larger of this and the tau carried in from the tiles before is used.
// Exact hit.  E_best == 0 ends the search of that range block in that chunk: theta becomes "never flagged".
// Padding.  Rows past N_d in the last domain tile are zero rows -- flagged while theta < 0 -- and are masked off before anything
// is evaluated; columns whose range block is >= N_r start at "never flagged", are masked as well, and write no slot.  Every
// (chunk, range block < N_r) writes its slot: a chunk has at least one real row.
//
// Registers.  B fragments of the wave's CTW = 4 / 2 / 1 column tiles stay in VGPRs (48 / 96 / 192 per lane).  A fragments are
// streamed in groups of G = min(NK, 12) K-steps with the next group in flight (at B = 16: 4 groups per domain tile), so that
// 192 + 2 * 48 + 16 stay inside the 512-entry unified file at one wave per SIMD.
//
// Shared code (fic_lsq_q_tile.h): the prep's fragment packers, the f16 pair / maximum helpers, the constants, the flagged mask
// and the 16 rounds (theta from tau, group minimum); fic_lsq_q_chunks.h: the chunk plan and the launcher's chunk conditions.
// The wave decode, the publish merge and the statistics are written out here and in fic_lsq_q.hip alike: shared, they cost
// sweep time.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "fic_device.h"
#include "fic_launch.h"
#include "fic_devfn.h"
#include "fic_lsq_rgb_fit.h"
#include "fic_lsq_q_chunks.h"
#include "fic_lsq_q_tile.h"

typedef uint32_t u32x8 __attribute__((ext_vector_type(8)));

#define FIC_LSQ_RGB_Q_ECOEF 7.0e-4f            // >= 2^-11 (1 + 2^-10) + 2^-22 with 2.1e-4 to spare (header)
#define FIC_LSQ_RGB_Q_EACC 1.1e-6f             // per K-step: >= 17 * 2^-24 * (1 + 2^-10)
#define FIC_LSQ_RGB_Q_ESUB 1.0575e-4f          // per unit of B: >= sqrt(3) * 2^-14 (subnormal entries, kept or flushed)

__host__ __device__ constexpr int lsq_rgb_q_ctw_nk(int NK) { return NK == 3 ? 4 : (NK == 12 ? 2 : 1); }

struct LsqRgbQArgs {
    const uint8_t* pool3;
    const u32x8* pool_st;
    const uint32_t* rng3;
    const u32x4* rng_st;
    const v4i* poolQ;          // A fragments [planes][ndtiles][NK][64]
    const v4i* rngQ;           // B fragments [planes][nct_alloc][NK][64]
    const float* rngE;         // Er [planes][Nr_pad]
    const uint32_t* rngR;      // R  [planes][Nr_pad]
    long long* slotE;          // [planes][nchunks][Nr_pad]
    uint32_t* slotC;
    int Nd, Nd_pad, Nr, Nr_pad, n_iso, lgn, planes;
    int nct;                   // column tiles: ceil(Nr * n_iso / 32)
    int nctg;                  // workgroups per (plane, chunk): ceil(nct / (WPG * CTW))
    int ndtiles, tiles_per_chunk, nchunks;
    unsigned long long* stats; // NULL, or "sweep_stats": {tile epilogues, tiles with flagged pairs, pairs evaluated exactly, waves}
    float tau_safety, tau_widen;
};

// rng3[plane][tile][k][w][lane], j = tile * 64 + lane (fic_lsq_rgb.hip's store)
__device__ __forceinline__ size_t lsq_rgb_q_rng3_index(int n_iso, int DW3, int j, int k, int w)
{
    return ((((size_t)(j >> 6)) * n_iso + k) * DW3 + w) * 64 + (j & 63);
}

// sum_ch S_r S_d, exact (< 2^34): fic_lsq_rgb.hip's lsq_rgb_cross
__device__ __forceinline__ long long lsq_rgb_q_cross(const uint32_t S_r[3], const uint32_t S_d[3])
{
    return (long long)S_r[0] * S_d[0] + (long long)S_r[1] * S_d[1] + (long long)S_r[2] * S_d[2];
}

// ---------------------------------------------------------------------------------------------
// k_lsq_rgb_q_prep : after k_lsq_rgb_prep.  Workgroups [0, ndtiles): the A fragments of one domain tile (32 pool blocks);
// [ndtiles, ndtiles + nct): the B fragments of one column tile (32 columns; zeros past N_r); the rest: R and Er of 256 range
// blocks each.  Fragment slot (m, lane) holds elements [16 m + 8 (lane >> 5), +8) of row / column lane & 31
// (fic_lsq_q_tile.h packs a slot); 8 consecutive elements lie in one channel (n is a multiple of 16).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_lsq_rgb_q_prep(const uint8_t* __restrict__ pool3, const u32x8* __restrict__ pool_st,
                                                        const uint32_t* __restrict__ rng3, const u32x4* __restrict__ rng_st,
                                                        v4i* __restrict__ poolQ, v4i* __restrict__ rngQ, float* __restrict__ rngE,
                                                        uint32_t* __restrict__ rngR, int B, int lgn, int Nd, int Nd_pad, int Nr,
                                                        int Nr_pad, int n_iso, int ndtiles, int nct, int eshift)
{
    const size_t plane = blockIdx.y;
    const int n = 1 << lgn, NK = 3 * n / 16, DW3 = 3 * n / 4;
    const int bx = (int)blockIdx.x;
    if (bx < ndtiles) {
        for (int t = threadIdx.x; t < NK * 64; t += 256) {
            const int lane = t & 63, m = t >> 6;
            const int d = bx * 32 + (lane & 31), p0 = 16 * m + 8 * (lane >> 5);
            v4i v = {0, 0, 0, 0};
            if (d < Nd) {
                const u32x8 ds = pool_st[plane * Nd_pad + d];
                if (ds[4] != 0u) {
                    const float w = __fdiv_rn(1.0f, __fmul_rn((float)B, __uint_as_float(ds[5])));
                    const int Sd = (int)ds[p0 >> lgn];
                    const uint2 pw = *(const uint2*)(pool3 + (plane * Nd_pad + d) * (size_t)(3 * n) + p0);
                    v = lsq_q_pack_pool(pw.x, pw.y, lgn, Sd, w);
                }
            }
            poolQ[(plane * ndtiles + bx) * NK * 64 + t] = v;
        }
    } else if (bx < ndtiles + nct) {
        const int ct = bx - ndtiles;
        const int cshift = n_iso == 8 ? 3 : 0;
        const uint32_t* rp = rng3 + plane * (size_t)Nr_pad * n_iso * DW3;
        for (int t = threadIdx.x; t < NK * 64; t += 256) {
            const int lane = t & 63, m = t >> 6;
            const int col = ct * 32 + (lane & 31), p0 = 16 * m + 8 * (lane >> 5);
            const int j = col >> cshift, k = col & (n_iso - 1);
            v4i v = {0, 0, 0, 0};
            if (j < Nr) {
                const u32x4 rs = rng_st[plane * Nr_pad + j];
                const int ch = p0 >> lgn;
                const int S_r = (int)(ch == 0 ? rs.x : (ch == 1 ? rs.y : rs.z));
                const int mr = (2 * S_r + n) >> (lgn + 1);
                const uint32_t w0 = rp[lsq_rgb_q_rng3_index(n_iso, DW3, j, k, p0 / 4)];
                const uint32_t w1 = rp[lsq_rgb_q_rng3_index(n_iso, DW3, j, k, p0 / 4 + 1)];
                v = lsq_q_pack_range(w0, w1, mr);
            }
            rngQ[(plane * nct + ct) * NK * 64 + t] = v;
        }
    } else {
        const int j = (bx - ndtiles - nct) * 256 + (int)threadIdx.x;
        if (j >= Nr_pad) return;
        const u32x4 rs = rng_st[plane * Nr_pad + j];                              // zeros for padding range blocks
        const int S[3] = {(int)rs.x, (int)rs.y, (int)rs.z};
        int ss = (int)rs.w;                                                       // sum (r - m_r)^2: exact, < 2^24 (header)
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const int mr = (2 * S[ch] + n) >> (lgn + 1);
            ss += mr * (n * mr - 2 * S[ch]);
        }
        const float c = __fadd_rn(__fadd_rn(FIC_LSQ_RGB_Q_ECOEF, __fmul_rn((float)NK, FIC_LSQ_RGB_Q_EACC)),
                                  __fmul_rn((float)B, FIC_LSQ_RGB_Q_ESUB));
        const float er = __fadd_rn(__fmul_rn(__fsqrt_rn((float)ss), c), FIC_LSQ_Q_EABS);
        rngE[plane * Nr_pad + j] = __fmul_rn(er, __int_as_float((127 - eshift) << 23));
        // n S_rr may pass 2^32 at B = 16; R < 2^31.6, so the difference modulo 2^32 is R: stored unsigned
        rngR[plane * Nr_pad + j] = (rs.w << lgn) - rs.x * rs.x - rs.y * rs.y - rs.z * rs.z;
    }
}

// ---------------------------------------------------------------------------------------------
// k_sweep_lsq_rgb_q<NK, CSHIFT> : NK = 3 n / 16 K-steps of v_mfma_f32_32x32x16_f16 per tile; 2^CSHIFT = n_iso columns per range
// block.  A wave owns CTW column tiles (their B fragments stay in VGPRs) and one pool chunk; it streams the chunk's domain tiles.
// Accumulator element e of lane l: column l & 31, domain row lsq_q_row(e, l >> 5) of the tile (fic_lsq_q_tile.h).
// ---------------------------------------------------------------------------------------------
template <int NK, int CSHIFT>
__global__ __launch_bounds__(64 * FIC_LSQ_RGB_Q_WPG, 1) void k_sweep_lsq_rgb_q(LsqRgbQArgs A)
{
    constexpr int CTW = lsq_rgb_q_ctw_nk(NK), CT = FIC_LSQ_RGB_Q_WPG * CTW;
    constexpr int NISO = 1 << CSHIFT, DW3 = NK * 4;
    constexpr int G = NK < 12 ? NK : 12, NG = NK / G;          // A fragments per group in flight, groups per domain tile
    constexpr bool WIDE = NK == 48;                            // B = 16: C and li in 64 bits (header, "Second stage")
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int combo_, gx_;
    xcd_decode(blockIdx.x, A.nchunks * A.planes, A.nctg, combo_, gx_);
    const int plane = combo_ / A.nchunks, chunk = combo_ % A.nchunks;
    const int ctw0 = gx_ * CT + wave * CTW;                    // first column tile of this wave
    const int dt0 = chunk * A.tiles_per_chunk;
    int dt1 = dt0 + A.tiles_per_chunk;
    if (dt1 > A.ndtiles) dt1 = A.ndtiles;
    if (ctw0 >= A.nct || dt0 >= dt1) return;                   // wave-uniform (the launcher makes no empty chunk)
    int nci = A.nct - ctw0;                                    // column tiles this wave really owns
    if (nci > CTW) nci = CTW;
    const int jcol = lane & 31, half = lane >> 5;

    // ---- this wave's columns: fragments and per-range state ---------------------------------
    v4i rb[CTW][NK];
    uint32_t S_r[CTW][3], S_rr[CTW], R[CTW], best_c[CTW], rbase[CTW];
    long long best_E[CTW];
    float theta[CTW], tau[CTW], Er[CTW];
    uint32_t okbits = 0;
    const uint32_t* rp = A.rng3 + (size_t)plane * A.Nr_pad * A.n_iso * DW3;
#pragma unroll
    for (int ci = 0; ci < CTW; ci++) {
        const int col = (ctw0 + ci) * 32 + jcol;
        const int j = col >> CSHIFT, k = col & (NISO - 1);
        const bool ok = ci < nci && j < A.Nr;
        const v4i* fp = A.rngQ + ((size_t)plane * A.nct + (ci < nci ? ctw0 + ci : ctw0)) * NK * 64 + lane;
#pragma unroll
        for (int m = 0; m < NK; m++) rb[ci][m] = ci < nci ? fp[m * 64] : v4i{0, 0, 0, 0};
        const size_t o = (size_t)plane * A.Nr_pad + (ok ? j : 0);
        const u32x4 st = A.rng_st[o];
        S_r[ci][0] = st.x;
        S_r[ci][1] = st.y;
        S_r[ci][2] = st.z;
        S_rr[ci] = st.w;
        R[ci] = A.rngR[o];
        Er[ci] = A.rngE[o];
        rbase[ci] = (uint32_t)lsq_rgb_q_rng3_index(A.n_iso, DW3, ok ? j : 0, k, 0);   // < 2^32 words per plane (the launcher checks)
        best_E[ci] = FIC_LSQ_E_NONE;
        best_c[ci] = 0xFFFFFFFFu;
        theta[ci] = ok ? -1.0f : FIC_LSQ_Q_NEVER;
        tau[ci] = -1.0f;
        okbits |= ok ? 1u << ci : 0u;
    }
    const float invB = NK == 3 ? 0.25f : (NK == 12 ? 0.125f : 0.0625f);
    unsigned st_tiles = 0, st_flagged = 0, st_pairs = 0;

    // tau of the column of tile ci from a smallest error E of its range block, -1 where T < 0: k_sweep_lsq_rgb_fast's chain, bit
    // for bit; theta follows from it by lsq_q_theta (the chain of the header)
    auto tau_of = [&](int ci, long long E) __attribute__((always_inline)) {
        const long long Ti = 1000000ll * (long long)R[ci] - (E << A.lgn);       // 10^6 T, exact
        return Ti < 0 ? -1.0f : __fmul_rn(__fmul_rn(__fmul_rn(sqrtf((float)Ti), 0.001f), A.tau_safety), A.tau_widen);
    };
    // exact evaluation of (column of tile ci, pool block d): the arithmetic of k_sweep_lsq_rgb_fast / _generic
    auto evaluate = [&](int ci, int d, float tl, long long& bE, uint32_t& bC) __attribute__((always_inline)) {
        const u32x8 ds = A.pool_st[(size_t)plane * A.Nd_pad + d];
        const uint4* pp = (const uint4*)(A.pool3 + ((size_t)plane * A.Nd_pad + d) * (size_t)(DW3 * 4));
        const uint32_t* rq = rp + rbase[ci];
        uint32_t acc = 0;                                      // <= 768 * 255^2 < 2^26
#pragma unroll 3
        for (int q = 0; q < DW3 / 4; q++) {
            const uint4 p4 = pp[q];
            acc = __builtin_amdgcn_udot4(rq[(4 * q + 0) * 64], p4.x, acc, false);
            acc = __builtin_amdgcn_udot4(rq[(4 * q + 1) * 64], p4.y, acc, false);
            acc = __builtin_amdgcn_udot4(rq[(4 * q + 2) * 64], p4.z, acc, false);
            acc = __builtin_amdgcn_udot4(rq[(4 * q + 3) * 64], p4.w, acc, false);
        }
        const uint32_t S_d[3] = {ds[0], ds[1], ds[2]};
        const float s32 = __uint_as_float(ds[5]);
        long long C;
        if constexpr (WIDE) {
            C = ((long long)acc << A.lgn) - lsq_rgb_q_cross(S_r[ci], S_d);
            const long long li = tl < 0.0f ? -1ll : (long long)__fmul_rn(tl, s32);
            if (C <= li && C >= -li) return;
        } else {
            const int C32 = (int)((acc << A.lgn) - (S_r[ci][0] * S_d[0] + S_r[ci][1] * S_d[1] + S_r[ci][2] * S_d[2]));
            const int li = tl < 0.0f ? -1 : (int)__fmul_rn(tl, s32);
            if (C32 <= li && C32 >= -li) return;
            C = (long long)C32;
        }
        const LsqRgbFit f = lsq_fit_rgb(A.lgn, S_r[ci], S_rr[ci], S_d, ds[3], acc, C, ds[4]);
        const uint32_t c = (uint32_t)d * (uint32_t)NISO + (uint32_t)(((ctw0 + ci) * 32 + jcol) & (NISO - 1));
        if (f.E < bE || (f.E == bE && c < bC)) {
            bE = f.E;
            bC = c;
        }
    };
    // A tile with |acc| above theta somewhere: evaluate what is flagged, then raise theta (header, "Ties" and "Within a tile")
    auto slow_tile = [&](const v16f& acc, int ci, int dt) __attribute__((always_inline)) {
        const bool ok = (okbits >> ci) & 1u;
        const uint32_t hm = lsq_q_flagged(acc, theta[ci], A.Nd - dt * 32, half, ok);
        if (__builtin_amdgcn_ballot_w64(hm != 0) == 0) return;
        st_flagged++;
        st_pairs += (unsigned)__builtin_popcount(hm);
        lsq_q_rounds<CSHIFT>(hm, dt * 32, half, ok, Er[ci], invB, theta[ci], tau[ci], best_E[ci], best_c[ci],
                             [&](int d, float tl, long long& bE, uint32_t& bC) __attribute__((always_inline)) { evaluate(ci, d, tl, bE, bC); },
                             [&](long long E) __attribute__((always_inline)) { return tau_of(ci, E); });
    };

    // ---- the sweep -----------------------------------------------------------------------------
    const v4i* pa = A.poolQ + (size_t)plane * A.ndtiles * NK * 64 + lane;
    const v16f zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    v4i an[G];
#pragma unroll
    for (int m = 0; m < G; m++) an[m] = pa[((size_t)dt0 * NK + m) * 64];
    for (int dt = dt0; dt < dt1; dt++) {
        v16f acc[CTW];
#pragma unroll
        for (int ci = 0; ci < CTW; ci++) acc[ci] = zero;
        const int dtn = dt + 1 < dt1 ? dt + 1 : dt;           // prefetch (the last trip reloads its own tile: nothing is over-read)
#pragma unroll
        for (int gq = 0; gq < NG; gq++) {
            v4i ac[G];
#pragma unroll
            for (int m = 0; m < G; m++) ac[m] = an[m];
            const size_t nxt = gq + 1 < NG ? (size_t)dt * NK + (size_t)(gq + 1) * G : (size_t)dtn * NK;
#pragma unroll
            for (int m = 0; m < G; m++) an[m] = pa[(nxt + m) * 64];
#pragma unroll
            for (int ci = 0; ci < CTW; ci++) {
#pragma unroll
                for (int m = 0; m < G; m++)
                    acc[ci] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, ac[m]),
                                                                     __builtin_bit_cast(f16x8, rb[ci][gq * G + m]), acc[ci], 0, 0, 0);
            }
        }
#pragma unroll
        for (int ci = 0; ci < CTW; ci++) {
            if (ci < nci) {
                st_tiles++;
                const float mx = max16_abs(acc[ci]);
                if (__builtin_amdgcn_ballot_w64(!(mx <= theta[ci])) != 0) slow_tile(acc[ci], ci, dt);
            }
        }
    }

    // ---- publish: this chunk's slot of every range block of the wave's column tiles ---------------
#pragma unroll
    for (int ci = 0; ci < CTW; ci++) {
        long long e = best_E[ci];
        uint32_t c = best_c[ci];
        auto merge = [&](int off) __attribute__((always_inline)) {
            const long long oe = __shfl_xor(e, off, 64);
            const uint32_t oc = __shfl_xor(c, off, 64);
            if (oe < e || (oe == e && oc < c)) {
                e = oe;
                c = oc;
            }
        };
        merge(32);
        if constexpr (CSHIFT == 3) {
            merge(1);
            merge(2);
            merge(4);
        }
        const int j = ((ctw0 + ci) * 32 + jcol) >> CSHIFT;
        if (((okbits >> ci) & 1u) && half == 0 && (jcol & (NISO - 1)) == 0) {
            const size_t o = ((size_t)plane * A.nchunks + chunk) * A.Nr_pad + j;
            A.slotE[o] = e;
            A.slotC[o] = c;
        }
    }
    if (A.stats) {
        atomicAdd(&A.stats[2], (unsigned long long)st_pairs);
        if (lane == 0) {
            atomicAdd(&A.stats[0], (unsigned long long)st_tiles);
            atomicAdd(&A.stats[1], (unsigned long long)st_flagged);
            atomicAdd(&A.stats[3], 1ull);
        }
    }
}

// host-side
int fic_launch_lsq_rgb_q_prep(const FicLsqRgb& q, const FicLsqRgbQ& s, const FicGeom& g, int eshift, hipStream_t st)
{
    if ((g.B != 4 && g.B != 8 && g.B != 16) || s.ndtiles != (g.Nd + 31) / 32 || s.nct < 1 || eshift < -12 || eshift > 4) return -1;
    const int nbr = (q.Nr_pad + 255) / 256;
    hipLaunchKernelGGL(k_lsq_rgb_q_prep, dim3(s.ndtiles + s.nct + nbr, g.planes), dim3(256), 0, st, (const uint8_t*)q.pool3,
                       (const u32x8*)q.pool_st, (const uint32_t*)q.rng3, (const u32x4*)q.rng_st, (v4i*)s.poolQ, (v4i*)s.rngQ,
                       (float*)s.rngE, (uint32_t*)s.rngR, g.B, g.lgn, g.Nd, g.Nd_pad, g.Nr, q.Nr_pad, g.n_iso, s.ndtiles, s.nct, eshift);
    FIC_LAUNCH_CHECK();
    return 0;
}

int fic_launch_sweep_lsq_rgb_q(const FicLsqRgb& q, const FicLsqRgbQ& s, const FicGeom& g, int tiles_per_chunk, int nchunks,
                               hipStream_t st, unsigned long long* stats, int tau_widen)
{
    if (!g.full || (g.B != 4 && g.B != 8 && g.B != 16) || (g.n_iso != 1 && g.n_iso != 8)) return -1;
    if ((long long)g.Nd * g.n_iso > 0xFFFFFFFEll) return -1;                       // c in 32 bits beside "none"
    if ((long long)q.Nr_pad * g.n_iso * 3 * g.DW >= (1ll << 32)) return -1;        // rbase: dword offsets within a plane
    if (s.ndtiles != (g.Nd + 31) / 32 || s.nct != (int)(((long long)g.Nr * g.n_iso + 31) / 32)) return -1;
    if (nchunks > FIC_LSQ_RGB_Q_MAX_CHUNKS || !lsq_q_chunks_cover(s.ndtiles, tiles_per_chunk, nchunks)) return -1;
    const int CT = FIC_LSQ_RGB_Q_WPG * lsq_rgb_q_ctw(g.B);
    LsqRgbQArgs A;
    A.pool3 = (const uint8_t*)q.pool3;
    A.pool_st = (const u32x8*)q.pool_st;
    A.rng3 = (const uint32_t*)q.rng3;
    A.rng_st = (const u32x4*)q.rng_st;
    A.poolQ = (const v4i*)s.poolQ;
    A.rngQ = (const v4i*)s.rngQ;
    A.rngE = (const float*)s.rngE;
    A.rngR = (const uint32_t*)s.rngR;
    A.slotE = (long long*)q.slotE;
    A.slotC = q.slotC;
    A.Nd = g.Nd; A.Nd_pad = g.Nd_pad; A.Nr = g.Nr; A.Nr_pad = q.Nr_pad; A.n_iso = g.n_iso; A.lgn = g.lgn; A.planes = g.planes;
    A.nct = s.nct;
    A.nctg = (s.nct + CT - 1) / CT;
    A.ndtiles = s.ndtiles;
    A.tiles_per_chunk = tiles_per_chunk;
    A.nchunks = nchunks;
    A.stats = stats;
    A.tau_safety = FIC_LSQ_TAU_SAFETY;
    A.tau_widen = fic_lsq_tau_widen(tau_widen);
    const long long nwg = (long long)nchunks * g.planes * A.nctg;
    if (nwg > 0x7FFFFFFFll) return -1;
    dim3 grid((unsigned)nwg, 1, 1), block(64 * FIC_LSQ_RGB_Q_WPG);
    const bool iso8 = g.n_iso == 8;
    if (g.B == 4 && !iso8) hipLaunchKernelGGL((k_sweep_lsq_rgb_q<3, 0>), grid, block, 0, st, A);
    else if (g.B == 4) hipLaunchKernelGGL((k_sweep_lsq_rgb_q<3, 3>), grid, block, 0, st, A);
    else if (g.B == 8 && !iso8) hipLaunchKernelGGL((k_sweep_lsq_rgb_q<12, 0>), grid, block, 0, st, A);
    else if (g.B == 8) hipLaunchKernelGGL((k_sweep_lsq_rgb_q<12, 3>), grid, block, 0, st, A);
    else if (!iso8) hipLaunchKernelGGL((k_sweep_lsq_rgb_q<48, 0>), grid, block, 0, st, A);
    else hipLaunchKernelGGL((k_sweep_lsq_rgb_q<48, 3>), grid, block, 0, st, A);
    FIC_LAUNCH_CHECK();
    return 0;
}
