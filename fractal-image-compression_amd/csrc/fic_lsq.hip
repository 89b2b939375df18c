// fic_lsq.hip -- least-squares domain search (option "search" = 1; an extension, the reference has no
// such criterion): k_lsq_stat, k_sweep_lsq_generic (any window, wave = range block), k_sweep_lsq_fast (full pool, lane = range
// block), k_finalize_lsq.  gfx950 (MI355X / CDNA4) only, wave64.
//
// For range block r and candidate d = pool block g read through isometry k (n = B*B, everything an exact integer):
//   S_r = sum r, S_rr = sum r^2, S_d = sum d, S_dd = sum d^2, S_rd = sum r d_k
//   C = n S_rd - S_r S_d,   V = n S_dd - S_d^2                                  (|C| <= sqrt(R V) < 2^31, 0 <= V < 2^31)
//   qa = 0 if V == 0 else clamp(floor((200 C + V) / (2 V)), -100, 100)           (100 C / V to nearest, then the clamp)
//   qb = floor((2 (100 S_r - qa S_d) + 100 n) / (200 n))                         (mean_r - qa mean_d / 100 to nearest)
//   E  = sum (100 r - qa d - 100 qb)^2
//      = 10^4 S_rr + qa^2 S_dd + 10^4 n qb^2 - 200 qa S_rd - 2 10^4 qb S_r + 200 qa qb S_d          (int64, >= 0)
// The winner is the smallest E, the first one in the order c = wloc * n_iso + k.  No float decides anything: the floats
// below only pick candidates that are then evaluated in integers, or skip candidates that provably cannot win.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "fic_device.h"
#include "fic_launch.h"
#include "fic_devfn.h"
#include "fic_lsq_fit.h"

// ---------------------------------------------------------------------------------------------
// k_lsq_stat : the sums the search needs beside k_pool's and k_range's.  Workgroups [0, nbp) take 256 pool blocks each:
// {S_d, S_dd, V, bits of (float) sqrt((double) V)} from pool_pix; the others 256 range blocks each: {S_r, S_rr} from copy 0 (the
// block itself) of the lane-transposed range store.  Padding range blocks get zeros.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_lsq_stat(const uint32_t* __restrict__ pool_pix, const uint32_t* __restrict__ rng_pix,
                                                  u32x4* __restrict__ lsq_pool, u32x2* __restrict__ lsq_rng, FicGeom g, int nbp)
{
    const int plane = blockIdx.y;
    if ((int)blockIdx.x < nbp) {
        const int d = blockIdx.x * 256 + threadIdx.x;
        if (d >= g.Nd) return;
        const uint32_t* pp = pool_pix + ((size_t)plane * g.Nd_pad + d) * g.DW;
        uint32_t S = 0, Q = 0;
        for (int dw = 0; dw < g.DW; dw++) {
            const uint32_t w = pp[dw];
            S = __builtin_amdgcn_sad_u8(w, 0u, S);
            Q = __builtin_amdgcn_udot4(w, w, Q, false);
        }
        const uint32_t V = (Q << g.lgn) - S * S;           // n S_dd <= 2^32 - 2^17 and S_d^2 < 2^32: the difference is exact
        u32x4 o;
        o.x = S;
        o.y = Q;
        o.z = V;
        o.w = __float_as_uint((float)__dsqrt_rn((double)V));
        lsq_pool[(size_t)plane * g.Nd_pad + d] = o;
    } else {
        const int j = ((int)blockIdx.x - nbp) * 256 + threadIdx.x;
        if (j >= g.Nr_pad) return;
        uint32_t S = 0, Q = 0;
        if (j < g.Nr) {
            const uint32_t* rp = rng_pix + (size_t)plane * g.Nr_pad * g.n_iso * g.DW;
            for (int dw = 0; dw < g.DW; dw++) {
                const uint32_t w = rp[rng_word_index(g, j, 0, dw)];
                S = __builtin_amdgcn_sad_u8(w, 0u, S);
                Q = __builtin_amdgcn_udot4(w, w, Q, false);
            }
        }
        u32x2 o;
        o.x = S;
        o.y = Q;
        lsq_rng[(size_t)plane * g.Nr_pad + j] = o;
    }
}

// ---------------------------------------------------------------------------------------------
// k_sweep_lsq_generic : exact evaluation of every candidate of a window, one wave per range block (the shape of
// k_sweep_generic).  Lanes stride over the wK*wK*n_iso candidates, keep a running (E, candidate) minimum and the wave takes
// the lexicographic minimum with xor-shuffles: the strict '<' scan in ascending candidate order.  Serves every wK and is the
// in-GPU cross-check of k_sweep_lsq_fast.  Result: slot 0 of the per-chunk slots (one slot per plane).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sweep_lsq_generic(const uint32_t* __restrict__ pool_pix, const u32x4* __restrict__ lsq_pool,
                                                           const uint32_t* __restrict__ rng_pix, const u32x2* __restrict__ lsq_rng,
                                                           long long* __restrict__ slotE, uint32_t* __restrict__ slotC, FicGeom g,
                                                           int r_begin, int r_count)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int jr = blockIdx.x * 4 + wave;
    const int plane = blockIdx.y;
    if (jr >= r_count) return;
    const int j = r_begin + jr;
    const uint32_t* pp = pool_pix + (size_t)plane * g.Nd_pad * g.DW;
    const u32x4* ps = lsq_pool + (size_t)plane * g.Nd_pad;
    const uint32_t* rp = rng_pix + (size_t)plane * g.Nr_pad * g.n_iso * g.DW;
    const u32x2 rs = lsq_rng[(size_t)plane * g.Nr_pad + j];
    const int ncand = g.wK * g.wK * g.n_iso;
    long long bestE = FIC_LSQ_E_NONE;
    uint32_t bestC = 0xFFFFFFFFu;
    for (int c = lane; c < ncand; c += 64) {
        const int wloc = c / g.n_iso, k = c % g.n_iso;
        const int gi = window_to_global(g, j, wloc);
        const u32x4 ds = ps[gi];
        uint32_t acc = 0;
        for (int dw = 0; dw < g.DW; dw++)
            acc = __builtin_amdgcn_udot4(rp[rng_word_index(g, j, k, dw)], pp[(size_t)gi * g.DW + dw], acc, false);
        const int C = (int)((acc << g.lgn) - rs.x * ds.x);
        const LsqFit f = lsq_fit(g.lgn, (int)rs.x, (int)rs.y, (int)ds.x, (int)ds.y, (int)acc, C, (int)ds.z);
        if (f.E < bestE) {                                 // c ascends within a lane
            bestE = f.E;
            bestC = (uint32_t)c;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const long long oE = __shfl_xor(bestE, off, 64);
        const uint32_t oC = __shfl_xor(bestC, off, 64);
        if (oE < bestE || (oE == bestE && oC < bestC)) {
            bestE = oE;
            bestC = oC;
        }
    }
    if (lane == 0) {
        slotE[(size_t)plane * g.Nr_pad + j] = bestE;
        slotC[(size_t)plane * g.Nr_pad + j] = bestC;
    }
}

// ---------------------------------------------------------------------------------------------
// k_sweep_lsq_fast : full-pool search (wK == Dw == Dh), the mapping of k_sweep_fast (fic_sweep.hip):
//   * lane = range block; its pixels (and isometry copies) stay in VGPRs: NR ranges x NC copies x DW dwords per lane;
//   * the pool is the wave-uniform operand, streamed through the scalar path (pixels and the 16-byte statistics) and fed to
//     v_dot4_u32_u8 as the SGPR source, double-buffered;
//   * every lane sees its candidates in ascending order, so the strict '<' tie rule is a per-lane running minimum.
//
// Prune.  For ANY (a, b) the squared error of a d + b over r is at least that of the continuous optimum:
//     E / 10^4  >=  (S_rr - S_r^2 / n) - C^2 / (n V)  =  (R - C^2 / V) / n,      R = n S_rr - S_r^2   (V > 0),
// and E / 10^4 >= R / n when V == 0 (then C == 0).  A later candidate wins only with E' < E_best, so it may be skipped when
//     10^4 (R - C'^2 / V') / n >= E_best   <=>   C'^2 <= T V',   T = (10^4 R - n E_best) / 10^4,
// provided T >= 0 (with T < 0 nothing is skipped: a flat block, C' = V' = 0, could still win).  The test per pair is
//     |C'| <= li,   li = (int) fl(tau * s32'),   s32' = fl32(sqrt(V')),   tau = sqrtf(fl32(10^4 T)) * 0.01f * (1 - 2^-18):
// 10^4 T is an exact integer; its conversion to f32 (2^-24, halved by the root), the root (at most 1 ulp, 2^-23), the two
// products of tau, the representation of 0.01f, s32' and the product tau * s32' (2^-24 each) add up to less than 2^-21, so
// li <= sqrt(T V') (1 - 2^-18) (1 + 2^-21) < sqrt(T V'), and C' is an integer compared exactly (tau * s32' < 2^30.1: the
// conversion to int truncates a non-negative float, never rounds up).  tau = -1 stands for T < 0 and "nothing evaluated yet":
// li = -1 flags every pair, so the first block of a chunk is always evaluated.  Only flagged pairs run the 64-bit epilogue.
// The factor 1 - 2^-18 is the kernel argument tau_safety; tau_widen is 1, or 1 + 2^-k under the diagnostic option
// "lsq_tau_widen" = k, which puts li ABOVE the derivation (wrong codebooks) so that tests can show their inputs notice.
//
// Chunks and isometry groups do not share a key: E needs up to 42 bits beside a 25-bit candidate.  Every (chunk, group)
// writes its lane minimum to a slot of its own; k_finalize_lsq takes the lexicographic (E, candidate) minimum over the slots,
// which does not depend on how the pool was cut.
// ---------------------------------------------------------------------------------------------
struct LsqSweepArgs {
    const uint32_t* pool_pix;
    const u32x4* lsq_pool;
    const uint32_t* rng_pix;
    const u32x2* lsq_rng;
    long long* slotE;
    uint32_t* slotC;
    int Nd, Nd_pad, Nr, Nr_pad, n_iso, lgn;
    int tile0, ntiles;         // tiles [tile0, tile0+ntiles) of 64*NR ranges
    int chunk_len, nchunks;    // domain chunk length (multiple of 2), number of chunks (none of them empty)
    int planes;
    unsigned long long* stats; // NULL, or counters ("sweep_stats"): {(wave, pool block) visits, visits that ran the exact epilogue,
                               //  pairs evaluated exactly, waves}
    float tau_safety;          // the safety factor of tau, 1 - 2^-18 (FIC_LSQ_TAU_SAFETY)
    float tau_widen;           // 1, or 1 + 2^-k under the option "lsq_tau_widen" = k: diagnostic, > 0 gives WRONG codebooks
};

template <int DW, int NR, int NC>
__global__ __launch_bounds__(256) void k_sweep_lsq_fast(LsqSweepArgs A)
{
    constexpr int SEG = DW < 16 ? DW : 16;     // dwords per scalar load
    constexpr int NSEG = DW / SEG;             // scalar loads per domain block (1, or 4 for B = 16)
    typedef uint32_t segv __attribute__((ext_vector_type(SEG)));

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ngroups = A.n_iso / NC;
    const int nslots = A.nchunks * ngroups;
    int combo_, bx_;
    xcd_decode(blockIdx.x, nslots * A.planes, (A.ntiles + 3) / 4, combo_, bx_);
    const int slot = combo_ % nslots, plane = combo_ / nslots;
    const int tl = bx_ * 4 + wave;
    if (tl >= A.ntiles) return;                        // wave-uniform
    const int tile = A.tile0 + tl;
    const int chunk = slot / ngroups;
    const int kbase = (slot % ngroups) * NC;

    const int d0 = chunk * A.chunk_len;
    int d1 = d0 + A.chunk_len;
    if (d1 > A.Nd) d1 = A.Nd;
    if (d0 >= d1) return;                              // (the launcher makes no empty chunk)

    // ---- this lane's range blocks -> VGPRs ------------------------------------------------
    uint32_t r[NR][NC][DW];
    uint32_t S_r[NR], S_rr[NR], R[NR];
    long long best_E[NR];
    uint32_t best_cand[NR];
    float tau[NR];
    {
        const uint32_t* rp = A.rng_pix + (size_t)plane * A.Nr_pad * A.n_iso * DW;
#pragma unroll
        for (int rs = 0; rs < NR; rs++) {
#pragma unroll
            for (int k = 0; k < NC; k++)
#pragma unroll
                for (int dw = 0; dw < DW; dw++)
                    r[rs][k][dw] = rp[((((size_t)tile * NR + rs) * A.n_iso + kbase + k) * DW + dw) * 64 + lane];
            const u32x2 st = A.lsq_rng[(size_t)plane * A.Nr_pad + ((size_t)tile * NR + rs) * 64 + lane];
            S_r[rs] = st.x;
            S_rr[rs] = st.y;
            R[rs] = (st.y << A.lgn) - st.x * st.x;     // n S_rr <= 2^32 - 2^17, S_r^2 < 2^32: exact, < 2^31
            best_E[rs] = FIC_LSQ_E_NONE;
            best_cand[rs] = 0xFFFFFFFFu;
            tau[rs] = -1.0f;
        }
    }

    // ---- scalar streams ---------------------------------------------------------------------
    const AS4 segv* px = (const AS4 segv*)(A.pool_pix + (size_t)plane * A.Nd_pad * DW);
    const AS4 u32x4* st = (const AS4 u32x4*)(A.lsq_pool + (size_t)plane * A.Nd_pad);

    uint32_t acc[NR][NC];
    uint32_t n_slow = 0, n_exact = 0;                  // "sweep_stats": counted inside the epilogue only

    auto dots = [&](const segv& p, int seg) {
#pragma unroll
        for (int w = 0; w < SEG; w++)
#pragma unroll
            for (int rs = 0; rs < NR; rs++)
#pragma unroll
                for (int k = 0; k < NC; k++)
                    acc[rs][k] = __builtin_amdgcn_udot4(r[rs][k][seg * SEG + w], p[w], acc[rs][k], false);
    };
    auto begin_domain = [&]() {
#pragma unroll
        for (int rs = 0; rs < NR; rs++)
#pragma unroll
            for (int k = 0; k < NC; k++) acc[rs][k] = 0;
    };
    // exact epilogue of one (range, copy, domain): strict '<' in ascending candidate order, then tau from the new best
    auto evaluate = [&](int rs, int k, int d, const u32x4& s, int C) {
        const LsqFit f = lsq_fit(A.lgn, (int)S_r[rs], (int)S_rr[rs], (int)s.x, (int)s.y, (int)acc[rs][k], C, (int)s.z);
        n_exact++;
        if (f.E < best_E[rs]) {
            best_E[rs] = f.E;
            best_cand[rs] = (uint32_t)d * (uint32_t)A.n_iso + (uint32_t)(kbase + k);
            const long long Ti = 10000ll * (long long)R[rs] - (f.E << A.lgn);        // 10^4 T, exact
            tau[rs] = Ti < 0 ? -1.0f : __fmul_rn(__fmul_rn(__fmul_rn(sqrtf((float)Ti), 0.01f), A.tau_safety), A.tau_widen);
        }
    };
    auto end_domain = [&](int d, const u32x4& s) {     // s = {S_d, S_dd, V, bits of s32}
        const float s32 = __uint_as_float(s.w);
        bool any = false;
        int li[NR];
        int C[NR][NC];
#pragma unroll
        for (int rs = 0; rs < NR; rs++) {
            li[rs] = tau[rs] < 0.0f ? -1 : (int)__fmul_rn(tau[rs], s32);
            const uint32_t base = __umul24(S_r[rs], s.x);                            // S_r S_d mod 2^32 (both < 2^17)
            int mx = -2147483647 - 1, mn = 2147483647;
#pragma unroll
            for (int k = 0; k < NC; k++) {
                C[rs][k] = (int)((acc[rs][k] << A.lgn) - base);
                mx = max(mx, C[rs][k]);
                mn = min(mn, C[rs][k]);
            }
            any |= (mx > li[rs]) | (mn < -li[rs]);
        }
        if (__builtin_expect(__any(any), 0)) {
            n_slow++;
#pragma unroll
            for (int rs = 0; rs < NR; rs++)
#pragma unroll
                for (int k = 0; k < NC; k++) {
                    // li is re-read from tau: an earlier copy of this block may just have raised it
                    const int l = tau[rs] < 0.0f ? -1 : (int)__fmul_rn(tau[rs], s32);
                    if (C[rs][k] > l || C[rs][k] < -l) evaluate(rs, k, d, s, C[rs][k]);
                }
        }
    };

    if constexpr (NSEG == 1) {
        // two domain blocks per trip, buffers A/B; chunk_len is even, the pool tail is zero-padded
        segv pa = px[d0];
        u32x4 sa = st[d0];
        for (int d = d0; d < d1; d += 2) {
            __builtin_amdgcn_s_waitcnt(0xC07F);        // lgkmcnt(0): buffer A landed
            segv pb = px[d + 1];
            u32x4 sb = st[d + 1];
            __builtin_amdgcn_sched_barrier(0);         // keep the prefetch issue above the dot4s
            begin_domain();
            dots(pa, 0);
            end_domain(d, sa);
            __builtin_amdgcn_s_waitcnt(0xC07F);        // buffer B landed
            pa = px[d + 2];
            sa = st[d + 2];
            __builtin_amdgcn_sched_barrier(0);
            if (d + 1 < d1) {
                begin_domain();
                dots(pb, 0);
                end_domain(d + 1, sb);
            }
        }
    } else {
        // B = 16: four 16-dword segments per domain block, buffers alternate A B A B
        segv pa = px[(size_t)d0 * NSEG];
        u32x4 sc = st[d0];
        for (int d = d0; d < d1; d++) {
            const size_t sbase = (size_t)d * NSEG;
            u32x4 sn;
            segv pb;
#pragma unroll
            for (int sgi = 0; sgi < NSEG; sgi += 2) {
                __builtin_amdgcn_s_waitcnt(0xC07F);
                pb = px[sbase + sgi + 1];
                __builtin_amdgcn_sched_barrier(0);
                if (sgi == 0) begin_domain();
                dots(pa, sgi);
                __builtin_amdgcn_s_waitcnt(0xC07F);
                pa = px[sbase + sgi + 2];              // last trip: first segment of block d+1
                if (sgi + 2 == NSEG) sn = st[d + 1];
                __builtin_amdgcn_sched_barrier(0);
                dots(pb, sgi + 1);
            }
            end_domain(d, sc);
            __builtin_amdgcn_s_waitcnt(0xC07F);
            sc = sn;
        }
    }

    // ---- publish: this (chunk, isometry group)'s slot ---------------------------------------------
#pragma unroll
    for (int rs = 0; rs < NR; rs++) {
        const int j = (tile * NR + rs) * 64 + lane;
        if (j < A.Nr) {
            const size_t o = ((size_t)plane * nslots + slot) * A.Nr_pad + j;
            A.slotE[o] = best_E[rs];
            A.slotC[o] = best_cand[rs];
        }
    }
    if (A.stats) {
        atomicAdd(&A.stats[2], (unsigned long long)n_exact);
        if (lane == 0) {
            atomicAdd(&A.stats[0], (unsigned long long)(d1 - d0));
            atomicAdd(&A.stats[1], (unsigned long long)n_slow);
            atomicAdd(&A.stats[3], 1ull);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// k_finalize_lsq : lexicographic (E, candidate) minimum over the nslots slots of a range block, then the winner's fit once
// more from its sums, and the result arrays / packed records in k_finalize's layouts: qrows = {idx_local, qa, qb} as they
// are, a = (float) qa / 100f and b = (float) qb (the decoder's own values, FC:373), err = (float) ((double) E / 1e4).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_finalize_lsq(const uint32_t* __restrict__ pool_pix, const u32x4* __restrict__ lsq_pool,
                                                      const uint32_t* __restrict__ rng_pix, const u32x2* __restrict__ lsq_rng,
                                                      const long long* __restrict__ slotE, const uint32_t* __restrict__ slotC,
                                                      int nslots, FicOutputs out, long long* __restrict__ E_out, FicGeom g,
                                                      int r_begin, int r_count)
{
    const int jr = blockIdx.x * 256 + threadIdx.x;
    const int plane = blockIdx.y;
    if (jr >= r_count) return;
    const int j = r_begin + jr;
    long long bestE = FIC_LSQ_E_NONE;
    uint32_t c = 0xFFFFFFFFu;
    for (int sl = 0; sl < nslots; sl++) {
        const size_t o = ((size_t)plane * nslots + sl) * g.Nr_pad + j;
        const long long e = slotE[o];
        const uint32_t cc = slotC[o];
        if (e < bestE || (e == bestE && cc < c)) {
            bestE = e;
            c = cc;
        }
    }
    const int ncand = g.wK * g.wK * g.n_iso;
    if (c >= (uint32_t)ncand) c = 0;                   // cannot happen (every slot holds a candidate of its chunk); stay in bounds
    const int wloc = (int)(c / (uint32_t)g.n_iso), k = (int)(c % (uint32_t)g.n_iso);
    const int gi = window_to_global(g, j, wloc);
    const uint32_t* pp = pool_pix + ((size_t)plane * g.Nd_pad + gi) * g.DW;
    const uint32_t* rp = rng_pix + (size_t)plane * g.Nr_pad * g.n_iso * g.DW;
    const u32x4 ds = lsq_pool[(size_t)plane * g.Nd_pad + gi];
    const u32x2 rs = lsq_rng[(size_t)plane * g.Nr_pad + j];
    uint32_t acc = 0;
    for (int dw = 0; dw < g.DW; dw++) acc = __builtin_amdgcn_udot4(rp[rng_word_index(g, j, k, dw)], pp[dw], acc, false);
    const int C = (int)((acc << g.lgn) - rs.x * ds.x);
    const LsqFit f = lsq_fit(g.lgn, (int)rs.x, (int)rs.y, (int)ds.x, (int)ds.y, (int)acc, C, (int)ds.z);
    const float a = __fdiv_rn((float)f.qa, 100.0f), b = (float)f.qb;
    const size_t o = (size_t)plane * g.Nr + j;
    out.qrows[3 * o + 0] = wloc;
    out.qrows[3 * o + 1] = f.qa;
    out.qrows[3 * o + 2] = f.qb;
    out.idx_local[o] = wloc;
    out.idx_global[o] = gi;
    out.iso[o] = k;
    out.a[o] = a;
    out.b[o] = b;
    out.err[o] = (float)((double)f.E / 1e4);
    E_out[o] = f.E;
    int32_t* rec = out.records + 6 * o;
    rec[0] = wloc;
    rec[1] = (int32_t)__float_as_uint(a);
    rec[2] = (int32_t)__float_as_uint(b);
    rec[3] = k;
    rec[4] = f.qa;
    rec[5] = f.qb;
}

// host-side launchers
int fic_lsq_slots(const FicGeom& g, int nchunks)
{
    int NR, NC;
    if (fic_fast_variant(g.B, g.n_iso, &NR, &NC)) return 0;
    return nchunks * (g.n_iso / NC);
}

int fic_launch_lsq_stat(const FicBuffers& b, const FicLsq& q, const FicGeom& g, hipStream_t s)
{
    const int nbp = (g.Nd + 255) / 256, nbr = (g.Nr_pad + 255) / 256;
    hipLaunchKernelGGL(k_lsq_stat, dim3(nbp + nbr, g.planes), dim3(256), 0, s, (const uint32_t*)b.pool_pix, (const uint32_t*)b.rng_pix,
                       (u32x4*)q.pool, (u32x2*)q.rng, g, nbp);
    FIC_LAUNCH_CHECK();
    return 0;
}

int fic_launch_sweep_lsq_generic(const FicBuffers& b, const FicLsq& q, const FicGeom& g, int r_begin, int r_count, hipStream_t s)
{
    hipLaunchKernelGGL(k_sweep_lsq_generic, dim3((r_count + 3) / 4, g.planes), dim3(256), 0, s, (const uint32_t*)b.pool_pix,
                       (const u32x4*)q.pool, (const uint32_t*)b.rng_pix, (const u32x2*)q.rng, (long long*)q.slotE, q.slotC, g, r_begin,
                       r_count);
    FIC_LAUNCH_CHECK();
    return 0;
}

// The instantiations are k_sweep_fast's (fic_fast_variant, fic_device.h).
int fic_launch_sweep_lsq_fast(const FicBuffers& b, const FicLsq& q, const FicGeom& g, int tile0, int ntiles, int chunk_len, int nchunks,
                              hipStream_t s, unsigned long long* stats, int tau_widen)
{
    LsqSweepArgs A;
    A.stats = stats;
    A.tau_safety = FIC_LSQ_TAU_SAFETY;
    A.tau_widen = fic_lsq_tau_widen(tau_widen);
    A.pool_pix = (const uint32_t*)b.pool_pix;
    A.lsq_pool = (const u32x4*)q.pool;
    A.rng_pix = b.rng_pix;
    A.lsq_rng = (const u32x2*)q.rng;
    A.slotE = (long long*)q.slotE;
    A.slotC = q.slotC;
    A.Nd = g.Nd; A.Nd_pad = g.Nd_pad; A.Nr = g.Nr; A.Nr_pad = g.Nr_pad; A.n_iso = g.n_iso; A.lgn = g.lgn;
    A.tile0 = tile0; A.ntiles = ntiles; A.chunk_len = chunk_len; A.nchunks = nchunks; A.planes = g.planes;
    int NR, NC;
    if (fic_fast_variant(g.B, g.n_iso, &NR, &NC) || NR != g.NR) return -1;
    if (!g.full || chunk_len < 2 || (chunk_len & 1) || (long long)chunk_len * (nchunks - 1) >= g.Nd || (long long)chunk_len * nchunks < g.Nd ||
        tile0 < 0 || ntiles < 1 || tile0 + ntiles > g.tiles)
        return -1;
    dim3 grid((unsigned)(nchunks * (g.n_iso / NC) * g.planes) * (unsigned)((ntiles + 3) / 4), 1, 1);
    dim3 block(256);
    if (g.B == 4 && g.n_iso == 1) hipLaunchKernelGGL((k_sweep_lsq_fast<4, 4, 1>), grid, block, 0, s, A);
    else if (g.B == 4) hipLaunchKernelGGL((k_sweep_lsq_fast<4, 1, 8>), grid, block, 0, s, A);
    else if (g.B == 8 && g.n_iso == 1) hipLaunchKernelGGL((k_sweep_lsq_fast<16, 2, 1>), grid, block, 0, s, A);
    else if (g.B == 8) hipLaunchKernelGGL((k_sweep_lsq_fast<16, 1, 8>), grid, block, 0, s, A);
    else if (g.B == 16 && g.n_iso == 1) hipLaunchKernelGGL((k_sweep_lsq_fast<64, 2, 1>), grid, block, 0, s, A);
    else hipLaunchKernelGGL((k_sweep_lsq_fast<64, 1, 2>), grid, block, 0, s, A);
    FIC_LAUNCH_CHECK();
    return 0;
}

int fic_launch_finalize_lsq(const FicBuffers& b, const FicOutputs& out, const FicLsq& q, int nslots, const FicGeom& g, int r_begin,
                            int r_count, hipStream_t s)
{
    hipLaunchKernelGGL(k_finalize_lsq, dim3((r_count + 255) / 256, g.planes), dim3(256), 0, s, (const uint32_t*)b.pool_pix,
                       (const u32x4*)q.pool, (const uint32_t*)b.rng_pix, (const u32x2*)q.rng, (const long long*)q.slotE,
                       (const uint32_t*)q.slotC, nslots, out, (long long*)q.E, g, r_begin, r_count);
    FIC_LAUNCH_CHECK();
    return 0;
}
