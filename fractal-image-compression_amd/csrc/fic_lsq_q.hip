// fic_lsq_q.hip -- the least-squares domain search ("search" = 1, DESIGN.md sections 4.19 and 4.21) on the matrix cores, opt-in
// by the context option "lsq_engine" = 1: k_lsq_q_prep (operand fragments, per-range allowance) and k_sweep_lsq_q<NK, CSHIFT>
// (prune GEMM + exact evaluation of the survivors).  gfx950 (MI355X / CDNA4) only, wave64.  Compile with -ffp-contract=off.
//
// As everywhere in this library the matrix core only decides which pairs can be SKIPPED.  Every pair that can win is evaluated
// by the integer arithmetic of fic_lsq.hip -- S_rd by v_dot4_u32_u8 from the u8 pixels, C = n S_rd - S_r S_d, lsq_fit
// (fic_lsq_fit.h) -- and the winner is the lexicographic (E, c) minimum, c = pool block * n_iso + isometry; the per-chunk minima
// go to the slots that k_finalize_lsq merges.  The codebook therefore has the bits of k_sweep_lsq_fast's; a float can only cause
// more exact evaluations, never fewer than the proof below allows.
//
// Operands (n = B^2; S_d, V = n S_dd - S_d^2 and s32 = fl32(sqrt((double) V)) from k_lsq_stat's lsq_pool):
//     A[d][i] = f16( fl((float)(n d_i - S_d) * w) ),   w = fl(1 / fl(B * s32))      (V == 0 or d >= N_d: the row is all zeros)
//     B[i][c] = f16( copy_k[i] - m_r ),                 m_r = floor((2 S_r + n) / (2 n)), the integer nearest S_r / n
// for column c = j * n_iso + k (8 adjacent columns per range block with 8 isometries); copy_k is the copy in rng_pix, so that
// sum_i copy_k[i] d[i] = S_rd(k).  The exact row x^[i] = (n d_i - S_d) / sqrt(n V) has unit 2-norm and sums to zero, hence
//     q = sum_i x^[i] (copy_k[i] - m_r) = (n S_rd - S_d S_r) / sqrt(n V) = C / sqrt(n V)
// whatever m_r is; the centring only keeps ||b|| small (the ROUNDED row no longer sums to zero, so the error grows with ||b||).
// B entries are integers in [-255, 255]: exact in f16.
//
// The bound.  (4.19) a candidate Y cannot beat E_best when C_Y^2 <= T V_Y, T = (10^4 R - n E_best) / 10^4 >= 0, R = n S_rr -
// S_r^2, i.e. when |q_Y| <= sqrt(T / n) (V_Y == 0: C_Y = 0 and the condition is T >= 0).  With |acc - q| <= Er (below) it is
// enough that |acc_Y| <= theta with theta + Er < sqrt(T / n).  Ti = 10^4 T is an exact int64 and sqrt(T / n) = sqrt(Ti) / (100 B):
//     tau = fl(fl(fl(fl(sqrt(fl(Ti))) * 0.01f) * (1 - 2^-18)) * widen),   theta = fl( tau * (1/B) - Er )   (times 1 + 2^-22 where negative).
// fl(Ti) errs by 2^-24 (2^-25 after the root), the root by at most 1 ulp (2^-23; __fsqrt_rn is correctly rounded here, the
// bound does not need it), 0.01f lies below 0.01, three roundings of products (the product with the power of two 1/B is exact)
// 2^-24 each: together < 2^-21, so the minuend a <= sqrt(T / n) (1 - 2^-18)(1 + 2^-21); the subtraction rounds by at most
// 2^-24 |a - Er|, which is <= 2^-24 a while a >= Er, so theta + Er <= a (1 + 2^-24) < sqrt(T / n) then.  With a < Er the
// difference is negative and can be large against a; it is multiplied by 1 + 2^-22, which moves it away from zero by more than
// the two roundings can have moved it towards zero: theta <= a - Er there (such a theta flags everything anyway; the factor only
// makes theta + Er < sqrt(T / n) hold for every T > 0, as tests/test_lsq_q_bound.py checks it).  1 - 2^-18 is the safety factor of 4.19
// (FIC_LSQ_TAU_SAFETY); `widen` is 1, or 1 + 2^-k under the diagnostic option "lsq_tau_widen" (WRONG codebooks).
// theta < 0 flags every pair, zeros included: theta = -1 stands for "nothing evaluated yet" and for T < 0 (then a flat block,
// C = V = 0, could still win), and a - Er < 0 lands there too.  A zero row (V == 0) gives acc == 0 exactly, which passes only
// theta >= 0, and theta >= 0 implies T >= 0: the right condition for such a candidate.
//
// Second stage.  tau is the tau of k_sweep_lsq_fast, from the same instructions.  A pair that the GEMM flags has its S_rd and
// C computed exactly, and is then dropped without the 64-bit fit when |C| <= li = (int) fl(tau * s32), the exact integer test of
// fic_lsq.hip with its proof (li < sqrt(T V)): about Er / sqrt(T / n) ~ 10^-3 of the candidates near the bound are flagged by the
// allowance alone, and on smooth range blocks, where sqrt(T / n) is not large against Er, most flagged pairs are.  It is also
// where "lsq_tau_widen" bites exactly as in k_sweep_lsq_fast; in theta the widening drowns in Er.
//
// Rounding allowance, Er = fl(fl(fl(sqrt(ss)) * c_B) + abs) * 2^-lsq_q_eshift, ss = sum (r_i - m_r)^2 = ||b||^2 (an exact integer
// < 2^24), c_B = 7.0e-4f + B * 2^-14, abs = 1.6e-5f:
//   * B * s32 is exact (a power of two times a float); s32 is the correctly rounded double root rounded once more (2^-24 (1 +
//     2^-29)), the divide and the product are correctly rounded (2^-24 each; the library is built without fast-math): the f32
//     value of x_i is within 2^-22 relative.
//   * f16 rounding: 2^-11 relative while |x_i| >= 2^-14.  A non-zero x_i is >= 1 / sqrt(n V) > 2^-19.5 (V < 2^31, n <= 256) and
//     so CAN fall below f16's smallest normal 2^-14 (it takes n V > 2^28: a high-variance block with a pixel next to its mean).
//     The conversion keeps such values as subnormals (hipcc's default kernel mode: f16 denormals on), absolute error <= 2^-25
//     each, and the MFMA takes f16 subnormal inputs as they are (CDNA3 ISA 7.4: the matrix instructions do not flush).  The
//     allowance does NOT rely on either: if all of them were flushed to zero the loss is at most sum_{|x_i| < 2^-14} |x_i| |b_i|
//     <= 2^-14 sum |b_i| <= 2^-14 B ||b||, which is the second term of c_B.  (Kept subnormals: <= 2^-25 B ||b|| <= 2^-21 ||b||.)
//   * products of an 8-bit and an 11-bit significand are exact in f32; the accumulation of NK * 16 terms inside the MFMAs adds at
//     most 2^-24 * 17 NK * sum |A||B| (fic_q.hip's header), sum |A||B| <= ||x|| ||b|| <= (1 + 2^-10) ||b||: < 2^-15.9 ||b||.
//   Total |acc - q| <= (2^-11 (1 + 2^-10) + 2^-22 + 2^-15.9 + 2^-21 + [2^-14 B]) ||b|| < (2^-11 * 1.04 + 2^-14 B) ||b||, against
//   c_B = 2^-11 * 1.43 + 2^-14 B: the difference, 1.9e-4 ||b||, and `abs` cover the three roundings of Er itself (and a root
//   that were 1 ulp low).  ||b|| = 0 means b = 0, acc = 0 = q.  tests/lsqqmodel.py restates the prep and tests/test_lsq_q_bound.py
//   checks |acc - q| + the accumulation term <= Er and theta + Er < sqrt(T / n) in exact arithmetic.
//
// Ties.  theta of a range block is only ever derived from E_best over pairs that HAVE been evaluated, all of them in domain
// tiles before the one under test (or, within a chunk's first tile, nothing: theta = -1).  The candidates of one domain tile
// are tested against the theta of the tiles before it, all flagged pairs of the tile are evaluated, each lane keeps the
// lexicographic (E, c) minimum of what it evaluated, and only then is theta raised from the minimum E over the lanes that share
// the range block.  So a pruned Y has E_Y >= E_best = E_X with c_X < c_Y (X in an earlier tile: a smaller pool index, hence a
// smaller c for any isometry): X wins the tie.  No seeding from a tile's largest |acc| and no bound shared between chunks: a
// chunk evaluates its first tile in full and the E_best + 1 rule of 4.19 is not needed.
// Within a tile (B = 16).  The flagged pairs of a tile are evaluated in 16 rounds (accumulator element e of every lane), which is not the
// order of c: a round holds rows r and r + 4, and later rounds hold rows below those of earlier ones.  Only tau, the second
// stage's bound, moves between the rounds, and it is computed from E_best + 1: a pair Y dropped by it has E_Y >= E_X + 1 > E_X
// for an evaluated X, so X beats Y in any index order and ties are not touched (4.19, point 3).  It is the running bound of
// k_sweep_lsq_fast at the granularity of a round: after the first rounds of a chunk's first tile most pairs skip the 64-bit fit.
// The larger of this and the tau carried in from the tiles before (valid for every candidate of the tile) is used.
// Queue (B = 4 / 8).  Evaluating a pair means dependent loads from L2 (statistics, 2 x n bytes), about a microsecond: done in the
// tile's own lanes, a round at a time, that latency is paid per flagged tile for a handful of pairs.  So at B = 4 / 8 the flagged
// pairs go to a queue in LDS (4 bytes: pool block relative to the chunk | column in wave << 22; filled in rounds of e with
// ballot / mbcnt, no atomics) and are evaluated one per lane, 64 at a time, when the queue holds FIC_LSQ_Q_QFLUSH of them and at
// the end of every domain tile.  The range blocks' minima are 64-bit keys in LDS, (E << 22) | (c - c of the chunk's first
// block), merged with an LDS atomic minimum: E < 2^42 (|100 r - qa d - 100 qb| <= 127 600, n <= 256) and the launcher keeps a
// chunk at 2^22 candidates at most; the unsigned order of the keys is the lexicographic order of (E, c).  Everything the queue
// holds is from the current domain tile and tau / theta were last raised before it: the argument of "Ties" holds as it stands,
// and there is no refinement within a tile.  B = 16 (128 bytes per block and copy, small pools) keeps the rounds.
// Exact hit.  E_best == 0 ends the search of that range block in that chunk (E >= 0, later candidates lose ties): theta becomes
// "never flagged".  Without it a flat range block (R = 0, theta < 0 forever) would evaluate the whole pool.
// Padding.  Rows past N_d in the last domain tile are zero rows -- flagged while theta < 0 -- and are masked off before
// anything is evaluated; columns whose range block is >= N_r (ragged last column tile) start at "never flagged", are masked as
// well, and write no slot.  Every (chunk, range block < N_r of a covered column tile) writes its slot: a chunk has at least one
// real row, and the group of lanes of a range block includes the lane that holds row 0 of the chunk's first tile.
//
// Cross-lane exchange: __shfl_xor (ds_bpermute) in B = 16's slow path and once at the end; ballots and LDS otherwise.
//
// Shared code (fic_lsq_q_tile.h): the prep's fragment packers, the f16 pair / maximum helpers, the constants, the flagged mask
// and B = 16's rounds (theta from tau, group minimum); fic_lsq_q_chunks.h: the launcher's chunk conditions.  The wave decode, the
// publish merge and the statistics are written out here and in fic_lsq_rgb_q.hip alike: shared, they cost sweep time (4.21).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "fic_device.h"
#include "fic_launch.h"
#include "fic_devfn.h"
#include "fic_lsq_fit.h"
#include "fic_lsq_q_chunks.h"
#include "fic_lsq_q_tile.h"

#define FIC_LSQ_Q_ECOEF 7.0e-4f            // >= 2^-10.5 (fic_q.hip's coefficient); + B * 2^-14 for flushed subnormals
#define FIC_LSQ_Q_QFLUSH 192               // B = 4 / 8: the queue is evaluated once it holds this many pairs (and after every domain tile)
#define FIC_LSQ_Q_WPG 4                    // waves per workgroup (independent: no barrier, no shared memory)

// column tiles (x32 columns) one wave keeps in registers: fic_q.hip's counts
__host__ __device__ constexpr int lsq_q_ctw(int NK) { return NK == 1 ? 8 : (NK == 4 ? 4 : 2); }

struct LsqQArgs {
    const uint8_t* pool_pix;
    const u32x4* lsq_pool;
    const uint32_t* rng_pix;
    const u32x2* lsq_rng;
    const v4i* poolQ;          // A fragments [planes][ndtiles][NK][64]
    const v4i* rngQ;           // B fragments [planes][nct_alloc][NK][64]
    const float* rngE;         // Er [planes][Nr_pad]
    const uint32_t* rngR;      // R  [planes][Nr_pad]
    long long* slotE;          // [planes][nchunks][Nr_pad]
    uint32_t* slotC;
    FicGeom g;
    int ct_begin, ct_end;      // column tiles of the range span
    int nctg;                  // workgroups per (plane, chunk): ceil((ct_end - ct_begin) / (WPG * CTW))
    int nct_alloc, ndtiles, tiles_per_chunk, nchunks;
    unsigned long long* stats; // NULL, or "sweep_stats": {tile epilogues, tiles with flagged pairs, pairs evaluated exactly, waves}
    float tau_safety, tau_widen;
};

// ---------------------------------------------------------------------------------------------
// k_lsq_q_prep : after k_pool, k_range (copies) and k_lsq_stat.  Workgroups [0, ndtiles): the A fragments of one domain tile
// (32 pool blocks); [ndtiles, ndtiles + nct_alloc): the B fragments of one column tile (32 columns; zeros past N_r);
// the rest: R and Er of 256 range blocks each.  Fragment slot (m, lane) holds elements [16 m + 8 (lane >> 5), +8) of row /
// column lane & 31 (fic_lsq_q_tile.h packs a slot).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_lsq_q_prep(const uint8_t* __restrict__ pool_pix, const u32x4* __restrict__ lsq_pool,
                                                    const uint32_t* __restrict__ rng_pix, const u32x2* __restrict__ lsq_rng,
                                                    v4i* __restrict__ poolQ, v4i* __restrict__ rngQ, float* __restrict__ rngE,
                                                    uint32_t* __restrict__ rngR, FicGeom g, int ndtiles, int nct_alloc, int eshift)
{
    const int plane = blockIdx.y;
    const int NK = g.n / 16;
    const int bx = (int)blockIdx.x;
    if (bx < ndtiles) {
        for (int t = threadIdx.x; t < NK * 64; t += 256) {
            const int lane = t & 63, m = t >> 6;
            const int d = bx * 32 + (lane & 31), p0 = 16 * m + 8 * (lane >> 5);
            v4i v = {0, 0, 0, 0};
            if (d < g.Nd) {
                const u32x4 ds = lsq_pool[(size_t)plane * g.Nd_pad + d];
                if (ds.z != 0u) {
                    const float w = __fdiv_rn(1.0f, __fmul_rn((float)g.B, __uint_as_float(ds.w)));
                    const uint2 pw = *(const uint2*)(pool_pix + ((size_t)plane * g.Nd_pad + d) * g.n + p0);
                    v = lsq_q_pack_pool(pw.x, pw.y, g.lgn, (int)ds.x, w);
                }
            }
            poolQ[((size_t)plane * ndtiles + bx) * NK * 64 + t] = v;
        }
    } else if (bx < ndtiles + nct_alloc) {
        const int ct = bx - ndtiles;
        const int cshift = g.n_iso == 8 ? 3 : 0;
        const uint32_t* rp = rng_pix + (size_t)plane * g.Nr_pad * g.n_iso * g.DW;
        for (int t = threadIdx.x; t < NK * 64; t += 256) {
            const int lane = t & 63, m = t >> 6;
            const int col = ct * 32 + (lane & 31), p0 = 16 * m + 8 * (lane >> 5);
            const int j = col >> cshift, k = col & (g.n_iso - 1);
            v4i v = {0, 0, 0, 0};
            if (j < g.Nr) {
                const int S_r = (int)lsq_rng[(size_t)plane * g.Nr_pad + j].x;
                const int mr = (2 * S_r + g.n) >> (g.lgn + 1);
                v = lsq_q_pack_range(rp[rng_word_index(g, j, k, p0 / 4)], rp[rng_word_index(g, j, k, p0 / 4 + 1)], mr);
            }
            rngQ[((size_t)plane * nct_alloc + ct) * NK * 64 + t] = v;
        }
    } else {
        const int j = (bx - ndtiles - nct_alloc) * 256 + (int)threadIdx.x;
        if (j >= g.Nr_pad) return;
        const u32x2 st = lsq_rng[(size_t)plane * g.Nr_pad + j];                  // zeros for padding range blocks
        const int S_r = (int)st.x, S_rr = (int)st.y;
        const int mr = (2 * S_r + g.n) >> (g.lgn + 1);
        const int ss = S_rr - 2 * mr * S_r + g.n * mr * mr;                      // sum (r - m_r)^2: exact, < 2^24
        const float c = __fadd_rn(FIC_LSQ_Q_ECOEF, __fmul_rn((float)g.B, 6.103515625e-05f));      // + B * 2^-14
        const float er = __fadd_rn(__fmul_rn(__fsqrt_rn((float)ss), c), FIC_LSQ_Q_EABS);
        rngE[(size_t)plane * g.Nr_pad + j] = __fmul_rn(er, __int_as_float((127 - eshift) << 23));
        rngR[(size_t)plane * g.Nr_pad + j] = (st.y << g.lgn) - st.x * st.x;      // n S_rr <= 2^32 - 2^17, S_r^2 < 2^32: exact, < 2^31
    }
}

// ---------------------------------------------------------------------------------------------
// k_sweep_lsq_q<NK, CSHIFT> : NK = n / 16 K-steps of v_mfma_f32_32x32x16_f16 per tile; 2^CSHIFT = n_iso columns per range block.
// A wave owns CTW column tiles (their B fragments stay in VGPRs) and one pool chunk; it streams the chunk's domain tiles.
// Accumulator element e of lane l: column l & 31, domain row lsq_q_row(e, l >> 5) of the tile (fic_lsq_q_tile.h).
// ---------------------------------------------------------------------------------------------
template <int NK, int CSHIFT>
__global__ __launch_bounds__(64 * FIC_LSQ_Q_WPG, NK == 1 ? 2 : 1) void k_sweep_lsq_q(LsqQArgs A)
{
    constexpr int CTW = lsq_q_ctw(NK), CT = FIC_LSQ_Q_WPG * CTW;
    constexpr int NISO = 1 << CSHIFT, DW = NK * 4;
    const FicGeom& g = A.g;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int combo_, gx_;
    xcd_decode(blockIdx.x, A.nchunks * g.planes, A.nctg, combo_, gx_);
    const int plane = combo_ / A.nchunks, chunk = combo_ % A.nchunks;
    const int ctw0 = A.ct_begin + gx_ * CT + wave * CTW;      // first column tile of this wave
    const int dt0 = chunk * A.tiles_per_chunk;
    int dt1 = dt0 + A.tiles_per_chunk;
    if (dt1 > A.ndtiles) dt1 = A.ndtiles;
    if (ctw0 >= A.ct_end || dt0 >= dt1) return;               // wave-uniform (the launcher makes no empty chunk)
    int nci = A.ct_end - ctw0;                                // column tiles this wave really owns
    if (nci > CTW) nci = CTW;
    const int jcol = lane & 31, half = lane >> 5;

    // ---- this wave's columns: fragments and per-range state ---------------------------------
    v4i rb[CTW][NK];
    int S_r[CTW], S_rr[CTW];
    uint32_t R[CTW], best_c[CTW], rbase[CTW];
    long long best_E[CTW];
    float theta[CTW], tau[CTW], Er[CTW];
    uint32_t okbits = 0;
    const uint32_t* rp = A.rng_pix + (size_t)plane * g.Nr_pad * g.n_iso * g.DW;
#pragma unroll
    for (int ci = 0; ci < CTW; ci++) {
        const int col = (ctw0 + ci) * 32 + jcol;
        const int j = col >> CSHIFT, k = col & (NISO - 1);
        const bool ok = ci < nci && j < g.Nr;
        const v4i* fp = A.rngQ + ((size_t)plane * A.nct_alloc + ctw0 + ci) * NK * 64 + lane;
#pragma unroll
        for (int m = 0; m < NK; m++) rb[ci][m] = ci < nci ? fp[m * 64] : v4i{0, 0, 0, 0};
        const size_t o = (size_t)plane * g.Nr_pad + (ok ? j : 0);
        const u32x2 st = A.lsq_rng[o];
        S_r[ci] = (int)st.x;
        S_rr[ci] = (int)st.y;
        R[ci] = A.rngR[o];
        Er[ci] = A.rngE[o];
        rbase[ci] = (uint32_t)rng_word_index(g, ok ? j : 0, k, 0);   // < 2^32 words per plane (the store is indexed by int elsewhere)
        best_E[ci] = FIC_LSQ_E_NONE;
        best_c[ci] = 0xFFFFFFFFu;
        theta[ci] = ok ? -1.0f : FIC_LSQ_Q_NEVER;
        tau[ci] = -1.0f;
        okbits |= ok ? 1u << ci : 0u;
    }
    const float invB = NK == 1 ? 0.25f : (NK == 4 ? 0.125f : 0.0625f);
    unsigned st_tiles = 0, st_flagged = 0, st_pairs = 0;

    // tau from 10^4 T = Ti >= 0: k_sweep_lsq_fast's chain, bit for bit
    auto tau_chain = [&](long long Ti) __attribute__((always_inline)) {
        return __fmul_rn(__fmul_rn(__fmul_rn(__fsqrt_rn((float)Ti), 0.01f), A.tau_safety), A.tau_widen);
    };
    // the queue's theta (and tau) of the column of tile ci from E_best > 0 of its range block: the chain of the header
    auto raise_theta = [&](int ci, long long Eg, float& tau_out) __attribute__((always_inline)) {
        const long long Ti = 10000ll * (long long)R[ci] - (Eg << g.lgn);        // 10^4 T, exact
        if (Ti < 0) {
            theta[ci] = -1.0f;
            tau_out = -1.0f;
        } else {
            tau_out = tau_chain(Ti);
            const float th = __fsub_rn(__fmul_rn(tau_out, invB), Er[ci]);       // tau / B is exact
            theta[ci] = th < 0.0f ? __fmul_rn(th, FIC_LSQ_Q_AWAY) : th;         // a < Er: rounded away from zero (header)
        }
    };

    // ---- B = 4 / 8: flagged pairs are queued and evaluated one per lane (header, "Queue") ----------------------------------
    constexpr bool QUEUE = NK != 16;
    constexpr int QCAP = FIC_LSQ_Q_QFLUSH + 1024, NRNG = (CTW * 32) >> CSHIFT;
    __shared__ uint32_t sQ[QUEUE ? FIC_LSQ_Q_WPG : 1][QUEUE ? QCAP : 1];
    __shared__ unsigned long long sBest[QUEUE ? FIC_LSQ_Q_WPG : 1][QUEUE ? NRNG : 1];      // (E << 22) | (c - c of the chunk's first block)
    __shared__ float sTau[QUEUE ? FIC_LSQ_Q_WPG : 1][QUEUE ? NRNG : 1];
    uint32_t* const myq = sQ[QUEUE ? wave : 0];
    unsigned long long* const myBest = sBest[QUEUE ? wave : 0];
    float* const myTau = sTau[QUEUE ? wave : 0];
    int qn = 0;                                               // queued entries (wave-uniform)
    uint32_t dirty = 0;                                       // bit ci: pairs of that column tile were queued since the last flush
    if constexpr (QUEUE) {
        for (int i = lane; i < NRNG; i += 64) {
            myBest[i] = ~0ull;
            myTau[i] = -1.0f;
        }
        __builtin_amdgcn_wave_barrier();
    }
    // entries of one (domain tile, column tile): pool block relative to the chunk | column in wave << 22, in rounds of e
    auto push_tile = [&](const v16f& acc, int ci, int dt) __attribute__((always_inline)) {
        const uint32_t hm = lsq_q_flagged(acc, theta[ci], g.Nd - dt * 32, half, (okbits >> ci) & 1u);
        if (__builtin_amdgcn_ballot_w64(hm != 0) == 0) return;
        st_flagged++;
        dirty |= 1u << ci;
        const uint32_t ent0 = (uint32_t)((dt - dt0) * 32 + 4 * half) | ((uint32_t)(ci * 32 + jcol) << 22);
#pragma unroll 1
        for (int e = 0; e < 16; e++) {
            const bool mine = (hm >> e) & 1u;
            const unsigned long long b = __builtin_amdgcn_ballot_w64(mine);
            if (b == 0) continue;
            if (mine) myq[qn + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u))] = ent0 + (uint32_t)lsq_q_row(e, 0);
            qn += __builtin_popcountll(b);
        }
    };
    auto flush = [&]() __attribute__((always_inline)) {
        __builtin_amdgcn_wave_barrier();
        st_pairs += (unsigned)qn;
        for (int base = 0; base < qn; base += 64) {
            const int i = base + lane;
            if (i < qn) {
                const uint32_t ent = myq[i];
                const int colw = (int)(ent >> 22), dl = (int)(ent & 0x3FFFFFu);
                const int d = dt0 * 32 + dl, col = ctw0 * 32 + colw;
                const int j = col >> CSHIFT, k = col & (NISO - 1), ridx = colw >> CSHIFT;
                const float tl = myTau[ridx];
                const u32x2 rs = A.lsq_rng[(size_t)plane * g.Nr_pad + j];
                const u32x4 ds = A.lsq_pool[(size_t)plane * g.Nd_pad + d];
                const uint4* pp = (const uint4*)(A.pool_pix + ((size_t)plane * g.Nd_pad + d) * (size_t)(DW * 4));
                const uint32_t* rq = rp + rng_word_index(g, j, k, 0);
                uint32_t sd = 0;
#pragma unroll
                for (int q = 0; q < DW / 4; q++) {
                    const uint4 p4 = pp[q];
                    sd = __builtin_amdgcn_udot4(rq[(4 * q + 0) * 64], p4.x, sd, false);
                    sd = __builtin_amdgcn_udot4(rq[(4 * q + 1) * 64], p4.y, sd, false);
                    sd = __builtin_amdgcn_udot4(rq[(4 * q + 2) * 64], p4.z, sd, false);
                    sd = __builtin_amdgcn_udot4(rq[(4 * q + 3) * 64], p4.w, sd, false);
                }
                const int C = (int)((sd << g.lgn) - rs.x * ds.x);
                const int li = tl < 0.0f ? -1 : (int)__fmul_rn(tl, __uint_as_float(ds.w));   // second stage (header)
                if (!(C <= li && C >= -li)) {
                    const LsqFit f = lsq_fit(g.lgn, (int)rs.x, (int)rs.y, (int)ds.x, (int)ds.y, (int)sd, C, (int)ds.z);
                    atomicMin(&myBest[ridx], ((unsigned long long)f.E << 22) | (unsigned long long)(uint32_t)(dl * NISO + k));
                }
            }
        }
        qn = 0;
        __builtin_amdgcn_wave_barrier();
        // theta / tau of the column tiles that had pairs in the queue, from the range blocks' new minima
#pragma unroll
        for (int ci = 0; ci < CTW; ci++) {
            if ((dirty >> ci) & 1u) {
                const int ridx = (ci * 32 + jcol) >> CSHIFT;
                const unsigned long long key = myBest[ridx];
                if (((okbits >> ci) & 1u) && key != ~0ull) {
                    float t = -1.0f;
                    if ((key >> 22) == 0) theta[ci] = FIC_LSQ_Q_NEVER;          // exact hit
                    else raise_theta(ci, (long long)(key >> 22), t);
                    myTau[ridx] = t;                                            // (every lane of the range block writes the same value)
                }
            }
        }
        dirty = 0;
        __builtin_amdgcn_wave_barrier();
    };

    // exact evaluation of (column of tile ci, pool block d): the arithmetic of k_sweep_lsq_fast
    auto evaluate = [&](int ci, int d, float tl, long long& bE, uint32_t& bC) __attribute__((always_inline)) {
        const u32x4 ds = A.lsq_pool[(size_t)plane * g.Nd_pad + d];
        const uint4* pp = (const uint4*)(A.pool_pix + ((size_t)plane * g.Nd_pad + d) * (size_t)(DW * 4));
        const uint32_t* rq = rp + rbase[ci];
        uint32_t acc = 0;
#pragma unroll 4
        for (int q = 0; q < DW / 4; q++) {
            const uint4 p4 = pp[q];
            acc = __builtin_amdgcn_udot4(rq[(4 * q + 0) * 64], p4.x, acc, false);
            acc = __builtin_amdgcn_udot4(rq[(4 * q + 1) * 64], p4.y, acc, false);
            acc = __builtin_amdgcn_udot4(rq[(4 * q + 2) * 64], p4.z, acc, false);
            acc = __builtin_amdgcn_udot4(rq[(4 * q + 3) * 64], p4.w, acc, false);
        }
        const int C = (int)((acc << g.lgn) - (uint32_t)S_r[ci] * ds.x);
        // second stage, k_sweep_lsq_fast's exact test on the integer C (header): spares the 64-bit fit of pairs that only Er flagged
        const int li = tl < 0.0f ? -1 : (int)__fmul_rn(tl, __uint_as_float(ds.w));
        if (C <= li && C >= -li) return;
        const LsqFit f = lsq_fit(g.lgn, S_r[ci], S_rr[ci], (int)ds.x, (int)ds.y, (int)acc, C, (int)ds.z);
        const uint32_t c = (uint32_t)d * (uint32_t)NISO + (uint32_t)(((ctw0 + ci) * 32 + jcol) & (NISO - 1));
        if (f.E < bE || (f.E == bE && c < bC)) {
            bE = f.E;
            bC = c;
        }
    };
    // A tile with |acc| above theta somewhere: evaluate what is flagged, then raise theta (header, "Ties" and "Within a tile")
    auto slow_tile = [&](const v16f& acc, int ci, int dt) __attribute__((always_inline)) {
        const bool ok = (okbits >> ci) & 1u;
        const uint32_t hm = lsq_q_flagged(acc, theta[ci], g.Nd - dt * 32, half, ok);
        if (__builtin_amdgcn_ballot_w64(hm != 0) == 0) return;
        st_flagged++;
        st_pairs += (unsigned)__builtin_popcount(hm);
        lsq_q_rounds<CSHIFT>(hm, dt * 32, half, ok, Er[ci], invB, theta[ci], tau[ci], best_E[ci], best_c[ci],
                             [&](int d, float tl, long long& bE, uint32_t& bC) __attribute__((always_inline)) { evaluate(ci, d, tl, bE, bC); },
                             [&](long long E) __attribute__((always_inline)) {           // tau of a smallest error E, -1 where T < 0
                                 const long long Ti = 10000ll * (long long)R[ci] - (E << g.lgn);
                                 return Ti < 0 ? -1.0f : tau_chain(Ti);
                             });
    };

    // ---- the sweep -----------------------------------------------------------------------------
    const v4i* pa = A.poolQ + (size_t)plane * A.ndtiles * NK * 64 + lane;
    const v16f zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    v4i an[NK];
#pragma unroll
    for (int m = 0; m < NK; m++) an[m] = pa[((size_t)dt0 * NK + m) * 64];
    for (int dt = dt0; dt < dt1; dt++) {
        v4i ac[NK];
#pragma unroll
        for (int m = 0; m < NK; m++) ac[m] = an[m];
        const int dtn = dt + 1 < dt1 ? dt + 1 : dt;           // prefetch (the last trip reloads its own tile: nothing is over-read)
#pragma unroll
        for (int m = 0; m < NK; m++) an[m] = pa[((size_t)dtn * NK + m) * 64];
#pragma unroll
        for (int ci = 0; ci < CTW; ci++) {
            if (ci < nci) {
                v16f acc = zero;
#pragma unroll
                for (int m = 0; m < NK; m++)
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, ac[m]), __builtin_bit_cast(f16x8, rb[ci][m]), acc, 0, 0, 0);
                st_tiles++;
                const float mx = max16_abs(acc);
                if (__builtin_amdgcn_ballot_w64(!(mx <= theta[ci])) != 0) {
                    if constexpr (QUEUE) {
                        push_tile(acc, ci, dt);
                        if (qn >= FIC_LSQ_Q_QFLUSH) flush();
                    } else {
                        slow_tile(acc, ci, dt);
                    }
                }
            }
        }
        if constexpr (QUEUE) {
            if (qn != 0) flush();                              // theta moves at the end of every domain tile at the latest
        }
    }

    // ---- publish: this chunk's slot of every range block of the wave's column tiles ---------------
#pragma unroll
    for (int ci = 0; ci < CTW; ci++) {
        long long e = best_E[ci];
        uint32_t c = best_c[ci];
        if constexpr (QUEUE) {
            const unsigned long long key = myBest[(ci * 32 + jcol) >> CSHIFT];
            if (key != ~0ull) {
                e = (long long)(key >> 22);
                c = (uint32_t)(key & 0x3FFFFFu) + (uint32_t)dt0 * 32u * (uint32_t)NISO;
            }
        }
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
            const size_t o = ((size_t)plane * A.nchunks + chunk) * g.Nr_pad + j;
            A.slotE[o] = e;
            A.slotC[o] = c;
        }
    }
    if (A.stats && lane == 0) {
        atomicAdd(&A.stats[0], (unsigned long long)st_tiles);
        atomicAdd(&A.stats[1], (unsigned long long)st_flagged);
        atomicAdd(&A.stats[3], 1ull);
    }
    if (A.stats && (!QUEUE || lane == 0)) atomicAdd(&A.stats[2], (unsigned long long)st_pairs);   // QUEUE: counted per wave
}

// host-side
int fic_lsq_q_ct(int B) { return FIC_LSQ_Q_WPG * lsq_q_ctw(B * B / 16); }

int fic_launch_lsq_q_prep(const FicBuffers& b, const FicLsq& q, const FicLsqQ& s, const FicGeom& g, int eshift, hipStream_t st)
{
    const int nbr = (g.Nr_pad + 255) / 256;
    hipLaunchKernelGGL(k_lsq_q_prep, dim3(s.ndtiles + s.nct_alloc + nbr, g.planes), dim3(256), 0, st, (const uint8_t*)b.pool_pix,
                       (const u32x4*)q.pool, (const uint32_t*)b.rng_pix, (const u32x2*)q.rng, (v4i*)s.poolQ, (v4i*)s.rngQ, (float*)s.rngE,
                       (uint32_t*)s.rngR, g, s.ndtiles, s.nct_alloc, eshift);
    FIC_LAUNCH_CHECK();
    return 0;
}

int fic_launch_sweep_lsq_q(const FicBuffers& b, const FicLsq& q, const FicLsqQ& s, const FicGeom& g, int ct_begin, int ct_end,
                           int tiles_per_chunk, int nchunks, hipStream_t st, unsigned long long* stats, int tau_widen)
{
    const int CT = fic_lsq_q_ct(g.B);
    if (!g.full || (g.B != 4 && g.B != 8 && g.B != 16) || (g.n_iso != 1 && g.n_iso != 8)) return -1;
    if (ct_begin < 0 || ct_end <= ct_begin || ct_end > s.nct_alloc || !lsq_q_chunks_cover(s.ndtiles, tiles_per_chunk, nchunks) ||
        tiles_per_chunk > fic_lsq_q_max_tiles_per_chunk(g.B, g.n_iso))
        return -1;
    LsqQArgs A;
    A.pool_pix = b.pool_pix;
    A.lsq_pool = (const u32x4*)q.pool;
    A.rng_pix = b.rng_pix;
    A.lsq_rng = (const u32x2*)q.rng;
    A.poolQ = (const v4i*)s.poolQ;
    A.rngQ = (const v4i*)s.rngQ;
    A.rngE = (const float*)s.rngE;
    A.rngR = (const uint32_t*)s.rngR;
    A.slotE = (long long*)q.slotE;
    A.slotC = q.slotC;
    A.g = g;
    A.ct_begin = ct_begin;
    A.ct_end = ct_end;
    A.nctg = (ct_end - ct_begin + CT - 1) / CT;
    A.nct_alloc = s.nct_alloc;
    A.ndtiles = s.ndtiles;
    A.tiles_per_chunk = tiles_per_chunk;
    A.nchunks = nchunks;
    A.stats = stats;
    A.tau_safety = FIC_LSQ_TAU_SAFETY;
    A.tau_widen = fic_lsq_tau_widen(tau_widen);
    dim3 grid((unsigned)(nchunks * g.planes) * (unsigned)A.nctg, 1, 1), block(64 * FIC_LSQ_Q_WPG);
    const bool iso8 = g.n_iso == 8;
    if (g.B == 4 && !iso8) hipLaunchKernelGGL((k_sweep_lsq_q<1, 0>), grid, block, 0, st, A);
    else if (g.B == 4) hipLaunchKernelGGL((k_sweep_lsq_q<1, 3>), grid, block, 0, st, A);
    else if (g.B == 8 && !iso8) hipLaunchKernelGGL((k_sweep_lsq_q<4, 0>), grid, block, 0, st, A);
    else if (g.B == 8) hipLaunchKernelGGL((k_sweep_lsq_q<4, 3>), grid, block, 0, st, A);
    else if (!iso8) hipLaunchKernelGGL((k_sweep_lsq_q<16, 0>), grid, block, 0, st, A);
    else hipLaunchKernelGGL((k_sweep_lsq_q<16, 3>), grid, block, 0, st, A);
    FIC_LAUNCH_CHECK();
    return 0;
}
