// fic_lsq_rgb.hip -- least-squares domain search of the joint-RGB path (option "search" = 1 of a colour context, DESIGN.md
// section 4.20; an extension, the reference has no such criterion): k_lsq_rgb_prep (planar byte stores and the sums),
// k_sweep_lsq_rgb_generic (any window, wave = range block), k_sweep_lsq_rgb_fast (full pool at B = 4 / 8, lane = range block),
// k_finalize_lsq_rgb.  gfx950 (MI355X / CDNA4) only, wave64.
//
// One a for the three channels, three b (the reference's row).  The definition and the fit are in fic_lsq_rgb_fit.h.  Only the
// channel SUMS of S_rr, S_dd and S_rd enter C, V and E, so a block is one vector of 3 n bytes (planar: R, G, B) and a pair
// costs one dot product over 3 n / 4 dwords.  The winner is the smallest E, the first one in the order c = wloc * n_iso + k.
// No float decides anything: the floats below only propose values that are then put right in integers, or skip candidates that
// provably cannot win.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "fic_device.h"
#include "fic_launch.h"
#include "fic_devfn.h"
#include "fic_lsq_rgb_fit.h"

#define FIC_LSQ_E_NONE 0x7FFFFFFFFFFFFFFFll

typedef uint32_t u32x8 __attribute__((ext_vector_type(8)));

// Address of dword w (0 .. 3 DW) of isometry copy k of range j in the lane-transposed colour range store:
//   rng3[plane][tile][k][w][lane],  j = tile * 64 + lane.
__device__ __forceinline__ size_t rng3_word_index(int n_iso, int DW3, int j, int k, int w)
{
    return ((((size_t)(j >> 6)) * n_iso + k) * DW3 + w) * 64 + (j & 63);
}

// ---------------------------------------------------------------------------------------------
// k_lsq_rgb_prep : the byte stores and the sums of the search.  Workgroups [0, nbp) take 256 pool blocks each: the block of
// createCodebuchRGB from the scaled image (k_scale_rgb's), unpacked to planar bytes pool3[d][ch][pos], and
// {S_d R, G, B, S_dd, V, bits of (float) sqrt((double) V), 0, 0}.  The others take 256 range blocks each: the isometry copies
// copy_k[pos] = r[src_{k^-1}(pos)] (sum_pos copy_k[pos] d[pos] = sum_i r[i] d[src_k(i)]) per channel into the
// lane-transposed store, and {S_r R, G, B, S_rr}.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_lsq_rgb_prep(const int32_t* __restrict__ argb, const int32_t* __restrict__ scaled,
                                                      uint8_t* __restrict__ pool3, u32x8* __restrict__ pool_st,
                                                      uint8_t* __restrict__ rng3, u32x4* __restrict__ rng_st, FicGeom g, int nbp,
                                                      int Nr_pad)
{
    const size_t plane = blockIdx.y;
    if ((int)blockIdx.x < nbp) {
        const int d = blockIdx.x * 256 + threadIdx.x;
        if (d >= g.Nd) return;
        const int c = d % g.Dw, r = d / g.Dw;
        const int32_t* src = scaled + plane * g.Ws * g.Hs + (size_t)(r * g.abstand) * g.Ws + c * g.abstand;
        uint8_t* pp = pool3 + (plane * g.Nd_pad + d) * 3 * g.n;
        uint32_t S[3] = {0, 0, 0}, Q = 0;
        for (int ry = 0; ry < g.B; ry++)
            for (int rx = 0; rx < g.B; rx++) {
                const int32_t v = src[(size_t)ry * g.Ws + rx];
                const int pos = rx + ry * g.B;
#pragma unroll
                for (int ch = 0; ch < 3; ch++) {
                    const uint32_t p = (uint32_t)(v >> (16 - 8 * ch)) & 0xffu;
                    pp[ch * g.n + pos] = (uint8_t)p;
                    S[ch] += p;
                    Q += p * p;
                }
            }
        // n S_dd may pass 2^32 at B = 16; V < 2^32 (3 n^2 255^2 / 4), so the difference modulo 2^32 is V
        const uint32_t V = (Q << g.lgn) - S[0] * S[0] - S[1] * S[1] - S[2] * S[2];
        u32x8 o;
        o[0] = S[0]; o[1] = S[1]; o[2] = S[2]; o[3] = Q; o[4] = V;
        o[5] = __float_as_uint((float)__dsqrt_rn((double)V));
        o[6] = 0; o[7] = 0;
        pool_st[plane * g.Nd_pad + d] = o;
    } else {
        const int j = ((int)blockIdx.x - nbp) * 256 + threadIdx.x;
        if (j >= g.Nr) return;
        const int32_t* im = argb + plane * g.W * g.H + (size_t)((j / g.Rw) * g.B) * g.W + (j % g.Rw) * g.B;
        uint8_t* rp = rng3 + plane * (size_t)Nr_pad * g.n_iso * 3 * g.n;
        const int DW3 = 3 * g.DW;
        uint32_t S[3] = {0, 0, 0}, Q = 0;
        for (int k = 0; k < g.n_iso; k++) {
            int ax, bx, cx, ay, by, cy;
            iso_affine(iso_inverse(k), g.B - 1, ax, bx, cx, ay, by, cy);
            for (int y = 0; y < g.B; y++)
                for (int x = 0; x < g.B; x++) {
                    const int pos = x + y * g.B;
                    const int sx = ax * x + bx * y + cx, sy = ay * x + by * y + cy;
                    const int32_t v = im[(size_t)sy * g.W + sx];
#pragma unroll
                    for (int ch = 0; ch < 3; ch++) {
                        const uint32_t p = (uint32_t)(v >> (16 - 8 * ch)) & 0xffu;
                        rp[rng3_word_index(g.n_iso, DW3, j, k, ch * g.DW + (pos >> 2)) * 4 + (pos & 3)] = (uint8_t)p;
                        if (k == 0) {
                            S[ch] += p;
                            Q += p * p;
                        }
                    }
                }
        }
        u32x4 o;
        o.x = S[0]; o.y = S[1]; o.z = S[2]; o.w = Q;
        rng_st[plane * Nr_pad + j] = o;
    }
}

// sum_ch S_r S_d, exact (< 2^34)
__device__ __forceinline__ long long lsq_rgb_cross(const uint32_t S_r[3], const uint32_t S_d[3])
{
    return (long long)S_r[0] * S_d[0] + (long long)S_r[1] * S_d[1] + (long long)S_r[2] * S_d[2];
}

// ---------------------------------------------------------------------------------------------
// k_sweep_lsq_rgb_generic : exact evaluation of every candidate of a window, one wave per range block (the shape of
// k_sweep_lsq_generic / k_sweep_rgb_iso).  Lanes stride over the wK*wK*n_iso candidates, keep a running (E, candidate) minimum
// and the wave takes the lexicographic minimum with xor-shuffles: the strict '<' scan in ascending candidate order.  Serves
// every wK, B and n_iso and is the in-GPU cross-check of k_sweep_lsq_rgb_fast.  Result: slot 0 of the per-chunk slots.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sweep_lsq_rgb_generic(const uint32_t* __restrict__ pool3, const u32x8* __restrict__ pool_st,
                                                               const uint32_t* __restrict__ rng3, const u32x4* __restrict__ rng_st,
                                                               long long* __restrict__ slotE, uint32_t* __restrict__ slotC, FicGeom g,
                                                               int Nr_pad)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + wave;
    const size_t plane = blockIdx.y;
    if (j >= g.Nr) return;
    const int DW3 = 3 * g.DW;
    const uint32_t* pp = pool3 + plane * g.Nd_pad * DW3;
    const u32x8* ps = pool_st + plane * g.Nd_pad;
    const uint32_t* rp = rng3 + plane * (size_t)Nr_pad * g.n_iso * DW3;
    const u32x4 rs = rng_st[plane * Nr_pad + j];
    const uint32_t S_r[3] = {rs.x, rs.y, rs.z};
    const uint32_t ncand = (uint32_t)(g.wK * g.wK) * (uint32_t)g.n_iso;
    long long bestE = FIC_LSQ_E_NONE;
    uint32_t bestC = 0xFFFFFFFFu;
    for (uint32_t c = (uint32_t)lane; c < ncand; c += 64) {
        const int wloc = (int)(c / (uint32_t)g.n_iso), k = (int)(c % (uint32_t)g.n_iso);
        const int gi = window_to_global(g, j, wloc);
        const u32x8 ds = ps[gi];
        const uint32_t S_d[3] = {ds[0], ds[1], ds[2]};
        uint32_t acc = 0;                                  // <= 768 * 255^2 < 2^26
        for (int w = 0; w < DW3; w++)
            acc = __builtin_amdgcn_udot4(rp[rng3_word_index(g.n_iso, DW3, j, k, w)], pp[(size_t)gi * DW3 + w], acc, false);
        const long long C = ((long long)acc << g.lgn) - lsq_rgb_cross(S_r, S_d);
        const LsqRgbFit f = lsq_fit_rgb(g.lgn, S_r, rs.w, S_d, ds[3], acc, C, ds[4]);
        if (f.E < bestE) {                                 // c ascends within a lane
            bestE = f.E;
            bestC = c;
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
        slotE[plane * Nr_pad + j] = bestE;
        slotC[plane * Nr_pad + j] = bestC;
    }
}

// ---------------------------------------------------------------------------------------------
// k_sweep_lsq_rgb_fast<DW3, NC> : full-pool search (wK == Dw == Dh) at B = 4 (DW3 = 12) and B = 8 (DW3 = 48), the mapping of
// k_sweep_lsq_fast:
//   * lane = range block; NC isometry copies of its 3 n bytes stay in VGPRs (NC * DW3 <= 96 dwords: all 8 copies at B = 4,
//     isometry groups of 2 at B = 8);
//   * the pool block and its 32-byte statistics are wave-uniform and come through the scalar loads; v_dot4_u32_u8 takes the
//     pool dword as its SGPR source;
//   * every lane sees its candidates in ascending order, so the strict '<' tie rule is a per-lane running minimum.
//
// Prune.  For ANY a and b_R, b_G, b_B the squared error over the three channels is at least that of the continuous optimum
// of one a and three free b: with R = sum_ch (n S_rr - S_r^2),
//     E / 10^6  >=  (R - 2 a C + a^2 V) / n  >=  (R - C^2 / V) / n     (V > 0),     E / 10^6 >= R / n  (V == 0, then C == 0).
// A later candidate wins only with E' < E_best, so it may be skipped when
//     10^6 (R - C'^2 / V') / n >= E_best   <=>   C'^2 <= T V',   T = (10^6 R - n E_best) / 10^6,
// provided T >= 0 (with T < 0 nothing is skipped).  The test per pair is
//     |C'| <= li,   li = (int) fl(tau * s32'),   s32' = fl32(sqrt(V')),   tau = sqrtf(fl32(10^6 T)) * 0.001f * (1 - 2^-18):
// 10^6 T is an exact integer below 2^48; its conversion to f32 (2^-24, halved by the root), the root (1 ulp, 2^-23), the two
// products of tau, the representation of 0.001f, s32' and the product tau * s32' (2^-24 each) add up to less than 2^-21, so
// li <= sqrt(T V') (1 - 2^-18) (1 + 2^-21) < sqrt(T V').  At B <= 8, R and V are at most 3 n^2 255^2 / 4 < 2^27.6, so
// |C| <= sqrt(R V) < 2^31: C is computed modulo 2^32 and read as a signed 32-bit integer, and tau * s32' < 2^27.6 converts to
// int without overflow (truncation of a non-negative float never rounds up).  Neither holds at B = 16 (|C| reaches 3.2e9,
// V needs the unsigned 32 bits): B = 16 runs through the generic kernel.  tau = -1 stands for T < 0 and "nothing evaluated
// yet": li = -1 flags every pair.  Only flagged pairs run the 64-bit epilogue.
// tau_safety and tau_widen (option "lsq_tau_widen": diagnostic, > 0 gives WRONG codebooks) are k_sweep_lsq_fast's.
//
// Every (pool chunk, isometry group) writes its lane minimum to a slot of its own; k_finalize_lsq_rgb takes the lexicographic
// (E, candidate) minimum over the slots, which does not depend on how the pool was cut.
// ---------------------------------------------------------------------------------------------
struct LsqRgbSweepArgs {
    const uint32_t* pool3;
    const u32x8* pool_st;
    const uint32_t* rng3;
    const u32x4* rng_st;
    long long* slotE;
    uint32_t* slotC;
    int Nd, Nd_pad, Nr, Nr_pad, n_iso, lgn;
    int ntiles;                // tiles of 64 ranges
    int chunk_len, nchunks;    // pool chunk length, number of chunks (none of them empty)
    unsigned long long* stats; // NULL, or counters ("sweep_stats"): {(wave, pool block) visits, visits that ran the exact epilogue,
                               //  pairs evaluated exactly, waves}
    float tau_safety;          // the safety factor of tau, 1 - 2^-18 (FIC_LSQ_TAU_SAFETY)
    float tau_widen;           // 1, or 1 + 2^-k under the option "lsq_tau_widen" = k: diagnostic, > 0 gives WRONG codebooks
};

template <int DW3, int NC>
__global__ __launch_bounds__(256) void k_sweep_lsq_rgb_fast(LsqRgbSweepArgs A)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tile = blockIdx.x * 4 + wave;
    if (tile >= A.ntiles) return;                      // wave-uniform
    const int ngroups = A.n_iso / NC;
    const int nslots = A.nchunks * ngroups;
    const int slot = blockIdx.y;
    const size_t plane = blockIdx.z;
    const int chunk = slot / ngroups;
    const int kbase = (slot % ngroups) * NC;
    const int d0 = chunk * A.chunk_len;
    int d1 = d0 + A.chunk_len;
    if (d1 > A.Nd) d1 = A.Nd;
    if (d0 >= d1) return;                              // (the launcher makes no empty chunk)

    // ---- this lane's range block -> VGPRs (lanes past N_r read the zeroed padding of the store) ----
    uint32_t r[NC][DW3];
    const int j = tile * 64 + lane;
    {
        const uint32_t* rp = A.rng3 + plane * (size_t)A.Nr_pad * A.n_iso * DW3;
#pragma unroll
        for (int k = 0; k < NC; k++)
#pragma unroll
            for (int w = 0; w < DW3; w++) r[k][w] = rp[(((size_t)tile * A.n_iso + kbase + k) * DW3 + w) * 64 + lane];
    }
    const u32x4 rs = A.rng_st[plane * A.Nr_pad + j];
    const uint32_t S_r[3] = {rs.x, rs.y, rs.z};
    const uint32_t R = (rs.w << A.lgn) - rs.x * rs.x - rs.y * rs.y - rs.z * rs.z;      // exact, < 2^28 at B <= 8
    long long best_E = FIC_LSQ_E_NONE;
    uint32_t best_cand = 0xFFFFFFFFu;
    float tau = -1.0f;
    const bool live = j < A.Nr;                        // the padding lanes of the last tile flag nothing and are not counted
    uint32_t n_slow = 0, n_exact = 0;                  // "sweep_stats": counted inside the epilogue only

    const AS4 uint32_t* px = (const AS4 uint32_t*)(A.pool3 + plane * A.Nd_pad * DW3);
    const AS4 u32x8* st = (const AS4 u32x8*)(A.pool_st + plane * A.Nd_pad);

    for (int d = d0; d < d1; d++) {
        const AS4 uint32_t* p = px + (size_t)d * DW3;
        const u32x8 s = st[d];
        uint32_t acc[NC];
#pragma unroll
        for (int k = 0; k < NC; k++) acc[k] = 0;
#pragma unroll
        for (int w = 0; w < DW3; w++) {
            const uint32_t pw = p[w];
#pragma unroll
            for (int k = 0; k < NC; k++) acc[k] = __builtin_amdgcn_udot4(r[k][w], pw, acc[k], false);
        }
        const float s32 = __uint_as_float(s[5]);
        const uint32_t base = rs.x * s[0] + rs.y * s[1] + rs.z * s[2];                 // sum_ch S_r S_d modulo 2^32
        int li = tau < 0.0f ? -1 : (int)__fmul_rn(tau, s32);
        int C[NC];
        int mx = -2147483647 - 1, mn = 2147483647;
#pragma unroll
        for (int k = 0; k < NC; k++) {
            C[k] = (int)((acc[k] << A.lgn) - base);
            mx = max(mx, C[k]);
            mn = min(mn, C[k]);
        }
        const bool any = live & ((mx > li) | (mn < -li));
        if (__builtin_expect(__any(any), 0)) {
            n_slow++;
            const uint32_t S_d[3] = {s[0], s[1], s[2]};
#pragma unroll
            for (int k = 0; k < NC; k++) {
                // li is re-read from tau: an earlier copy of this block may just have raised it
                li = tau < 0.0f ? -1 : (int)__fmul_rn(tau, s32);
                if (C[k] > li || C[k] < -li) {
                    const LsqRgbFit f = lsq_fit_rgb(A.lgn, S_r, rs.w, S_d, s[3], acc[k], (long long)C[k], s[4]);
                    n_exact += live ? 1u : 0u;
                    if (f.E < best_E) {
                        best_E = f.E;
                        best_cand = (uint32_t)d * (uint32_t)A.n_iso + (uint32_t)(kbase + k);
                        const long long Ti = 1000000ll * (long long)R - (f.E << A.lgn);          // 10^6 T, exact
                        tau = Ti < 0 ? -1.0f : __fmul_rn(__fmul_rn(__fmul_rn(sqrtf((float)Ti), 0.001f), A.tau_safety), A.tau_widen);
                    }
                }
            }
        }
    }

    if (j < A.Nr) {
        const size_t o = (plane * nslots + slot) * A.Nr_pad + j;
        A.slotE[o] = best_E;
        A.slotC[o] = best_cand;
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
// k_finalize_lsq_rgb : lexicographic (E, candidate) minimum over the nslots slots of a range block, then the winner's fit once
// more from its sums, and the result arrays of k_finalize_rgb: qrows5 = {idx_local, 1000 qa, 1000 t_R, 1000 t_G, t_B} as they
// are, a / bR / bG / bB what the decoder makes of that row (rgb_row_coef), iso (n_iso = 8 contexts) and E.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_finalize_lsq_rgb(const uint32_t* __restrict__ pool3, const u32x8* __restrict__ pool_st,
                                                          const uint32_t* __restrict__ rng3, const u32x4* __restrict__ rng_st,
                                                          const long long* __restrict__ slotE, const uint32_t* __restrict__ slotC,
                                                          int nslots, FicRgbOutputs out, long long* __restrict__ E_out, FicGeom g,
                                                          int Nr_pad)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    const size_t plane = blockIdx.y;
    if (j >= g.Nr) return;
    long long bestE = FIC_LSQ_E_NONE;
    uint32_t c = 0xFFFFFFFFu;
    for (int sl = 0; sl < nslots; sl++) {
        const size_t o = (plane * nslots + sl) * Nr_pad + j;
        const long long e = slotE[o];
        const uint32_t cc = slotC[o];
        if (e < bestE || (e == bestE && cc < c)) {
            bestE = e;
            c = cc;
        }
    }
    const uint32_t ncand = (uint32_t)(g.wK * g.wK) * (uint32_t)g.n_iso;
    if (c >= ncand) c = 0;                             // cannot happen (every slot holds a candidate of its chunk); stay in bounds
    const int wloc = (int)(c / (uint32_t)g.n_iso), k = (int)(c % (uint32_t)g.n_iso);
    const int gi = window_to_global(g, j, wloc);
    const int DW3 = 3 * g.DW;
    const uint32_t* pp = pool3 + (plane * g.Nd_pad + gi) * DW3;
    const uint32_t* rp = rng3 + plane * (size_t)Nr_pad * g.n_iso * DW3;
    const u32x8 ds = pool_st[plane * g.Nd_pad + gi];
    const u32x4 rs = rng_st[plane * Nr_pad + j];
    const uint32_t S_r[3] = {rs.x, rs.y, rs.z}, S_d[3] = {ds[0], ds[1], ds[2]};
    uint32_t acc = 0;
    for (int w = 0; w < DW3; w++) acc = __builtin_amdgcn_udot4(rp[rng3_word_index(g.n_iso, DW3, j, k, w)], pp[w], acc, false);
    const long long C = ((long long)acc << g.lgn) - lsq_rgb_cross(S_r, S_d);
    const LsqRgbFit f = lsq_fit_rgb(g.lgn, S_r, rs.w, S_d, ds[3], acc, C, ds[4]);
    const int q1 = 1000 * f.qa, q2 = 1000 * f.t[0], q3 = 1000 * f.t[1], q4 = f.t[2];   // |t| <= 51001: 32 bits
    const FicRgbCoef cf = rgb_row_coef(q1, q2, q3, q4);
    const size_t o = plane * g.Nr + j;
    out.qrows[5 * o + 0] = wloc;
    out.qrows[5 * o + 1] = q1;
    out.qrows[5 * o + 2] = q2;
    out.qrows[5 * o + 3] = q3;
    out.qrows[5 * o + 4] = q4;
    out.idx_local[o] = wloc;
    out.idx_global[o] = gi;
    if (out.iso) out.iso[o] = k;
    out.a[o] = cf.a;
    out.bR[o] = cf.bR;
    out.bG[o] = cf.bG;
    out.bB[o] = cf.bB;
    E_out[o] = f.E;
}

// host-side launchers
int fic_lsq_rgb_variant(int B, int n_iso, int* NC)
{
    if ((B != 4 && B != 8) || (n_iso != 1 && n_iso != 8)) return -1;
    if (NC) *NC = n_iso == 1 ? 1 : (B == 4 ? 8 : 2);
    return 0;
}

int fic_lsq_rgb_slots(const FicGeom& g, int nchunks)
{
    int NC;
    if (fic_lsq_rgb_variant(g.B, g.n_iso, &NC)) return 0;
    return nchunks * (g.n_iso / NC);
}

// scaleImageRGB of every plane (k_scale_rgb's launcher is the caller's), then the stores and sums
int fic_launch_lsq_rgb_prep(const int32_t* argb, const int32_t* scaled, const FicLsqRgb& q, const FicGeom& g, hipStream_t s)
{
    const int nbp = (g.Nd + 255) / 256, nbr = (g.Nr + 255) / 256;
    hipLaunchKernelGGL(k_lsq_rgb_prep, dim3(nbp + nbr, g.planes), dim3(256), 0, s, argb, scaled, (uint8_t*)q.pool3, (u32x8*)q.pool_st,
                       (uint8_t*)q.rng3, (u32x4*)q.rng_st, g, nbp, q.Nr_pad);
    FIC_LAUNCH_CHECK();
    return 0;
}

int fic_launch_sweep_lsq_rgb_generic(const FicLsqRgb& q, const FicGeom& g, hipStream_t s)
{
    hipLaunchKernelGGL(k_sweep_lsq_rgb_generic, dim3((g.Nr + 3) / 4, g.planes), dim3(256), 0, s, (const uint32_t*)q.pool3,
                       (const u32x8*)q.pool_st, (const uint32_t*)q.rng3, (const u32x4*)q.rng_st, (long long*)q.slotE, q.slotC, g, q.Nr_pad);
    FIC_LAUNCH_CHECK();
    return 0;
}

int fic_launch_sweep_lsq_rgb_fast(const FicLsqRgb& q, const FicGeom& g, int chunk_len, int nchunks, hipStream_t s,
                                  unsigned long long* stats, int tau_widen)
{
    int NC;
    if (fic_lsq_rgb_variant(g.B, g.n_iso, &NC) || !g.full) return -1;
    if (chunk_len < 1 || nchunks < 1 || (long long)chunk_len * (nchunks - 1) >= g.Nd || (long long)chunk_len * nchunks < g.Nd) return -1;
    const int nslots = nchunks * (g.n_iso / NC);
    if (nslots > 65535 || g.planes > 65535) return -1;
    LsqRgbSweepArgs A;
    A.pool3 = (const uint32_t*)q.pool3;
    A.pool_st = (const u32x8*)q.pool_st;
    A.rng3 = (const uint32_t*)q.rng3;
    A.rng_st = (const u32x4*)q.rng_st;
    A.slotE = (long long*)q.slotE;
    A.slotC = q.slotC;
    A.Nd = g.Nd; A.Nd_pad = g.Nd_pad; A.Nr = g.Nr; A.Nr_pad = q.Nr_pad; A.n_iso = g.n_iso; A.lgn = g.lgn;
    A.ntiles = q.Nr_pad / 64; A.chunk_len = chunk_len; A.nchunks = nchunks;
    A.stats = stats;
    A.tau_safety = FIC_LSQ_TAU_SAFETY;
    A.tau_widen = fic_lsq_tau_widen(tau_widen);
    dim3 grid((unsigned)((A.ntiles + 3) / 4), (unsigned)nslots, (unsigned)g.planes);
    dim3 block(256);
    if (g.B == 4 && g.n_iso == 1) hipLaunchKernelGGL((k_sweep_lsq_rgb_fast<12, 1>), grid, block, 0, s, A);
    else if (g.B == 4) hipLaunchKernelGGL((k_sweep_lsq_rgb_fast<12, 8>), grid, block, 0, s, A);
    else if (g.n_iso == 1) hipLaunchKernelGGL((k_sweep_lsq_rgb_fast<48, 1>), grid, block, 0, s, A);
    else hipLaunchKernelGGL((k_sweep_lsq_rgb_fast<48, 2>), grid, block, 0, s, A);
    FIC_LAUNCH_CHECK();
    return 0;
}

int fic_launch_finalize_lsq_rgb(const FicRgbOutputs& out, const FicLsqRgb& q, int nslots, const FicGeom& g, hipStream_t s)
{
    hipLaunchKernelGGL(k_finalize_lsq_rgb, dim3((g.Nr + 255) / 256, g.planes), dim3(256), 0, s, (const uint32_t*)q.pool3,
                       (const u32x8*)q.pool_st, (const uint32_t*)q.rng3, (const u32x4*)q.rng_st, (const long long*)q.slotE,
                       (const uint32_t*)q.slotC, nslots, out, (long long*)q.E, g, q.Nr_pad);
    FIC_LAUNCH_CHECK();
    return 0;
}
