// fic_launch.h -- internal: device buffer bundles + the kernel launchers of fic_prep / fic_sweep / fic_mfma /
// fic_decode / fic_rgb .hip, as called by fic_capi.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fic_device.h"
#include "fic_qt_decode_plan.h"

// Device-resident working set of one context (all planes of the batch).
//   pool_pix : u8  [planes][Nd_pad][n]    expanded domain pool, block pixels row-major (FC:1036), 64-B aligned
//   pool_st  :     [planes][Nd_pad]       {sum, (float)sqrt(var)}  -- streamed beside the pixels
//   pool_var : u32 [planes][Nd_pad]       Domainblock.variance (exact integer)
//   pool_s64 : f64 [planes][Nd_pad]       Math.sqrt((double) variance)
//   rng_pix  : u32 [planes][tiles][NR][n_iso][DW][64]   lane-transposed range blocks + isometry copies
//   rng_st   :     [planes][Nr_pad]       {rM, rem}
//   key      : u64 [planes][Nr_pad]       (orderable error << 32) | candidate
struct FicBuffers {
    uint8_t* gray;
    uint8_t* scaled;
    uint8_t* pool_pix;
    FicDomStat* pool_st;
    uint32_t* pool_var;
    double* pool_s64;
    uint32_t* rng_pix;
    FicRngStat* rng_st;
    unsigned long long* key;
};

// Per-range results, [planes][Nr] each (qrows: [planes][Nr][3]).
struct FicOutputs {
    int32_t* idx_local;   // window-local index  = imageInfo[j][0]   (FC:156, 629)
    int32_t* idx_global;  // pool index          = calculateIndices  (FC:853-893)
    int32_t* iso;         // winning isometry (0 when n_iso == 1)
    float* a;             // unquantised contrast   imageInfo[j][1]
    float* b;             // unquantised brightness imageInfo[j][2]
    float* err;           // winning error (diagnostic)
    int32_t* qrows;       // writeData rows: (int)idx, (int)(a*100), (int)b   (FC:242-244)
    int32_t* records;     // [planes][Nr][6] {idx_local, a bits, b bits, iso, (int)(a*100), (int)b}: the unit of the multi-GPU gather
};

#ifdef __HIPCC__
#include "fic_devfn.h"
// The tail of getBestDomainblock (FC:634-642: a = cov / varD, clamp, b = rM - a dM, never fused) + writeData's quantiser (FC:242-244)
// + the packed 24-byte record, for range j whose winner is (window-local wloc, pool block gi, isometry k); acc = sum copy_k[pos] d[pos].
// Shared by k_finalize and by the sweep's fused tail (fic_q.hip).
__device__ __forceinline__ void finalize_store(const FicOutputs& out, const FicGeom& g, int plane, int j, unsigned long long kk, int wloc,
                                               int gi, int k, uint32_t acc, FicDomStat ds, FicRngStat rs, uint32_t varu)
{
    int dM = (int)(ds.sum >> g.lgn);
    int cov = (int)acc - rs.rM * (int)ds.sum - dM * rs.rem;
    float var = (float)varu;
    float a = __fdiv_rn((float)cov, var);              // FC:634  (0/0 -> NaN when a flat block wins)
    if (a < -1.0f) a = -1.0f;                          // FC:636-639 (NaN passes through)
    else if (a > 1.0f) a = 1.0f;
    float b = __fsub_rn((float)rs.rM, __fmul_rn(a, (float)dM));   // FC:641, never fused
    size_t o = (size_t)plane * g.Nr + j;
    const int qa = java_f2i(__fmul_rn(a, 100.0f)), qb = java_f2i(b);
    out.qrows[3 * o + 0] = wloc;                       // (int) imageInfo[row][0]
    out.qrows[3 * o + 1] = qa;
    out.qrows[3 * o + 2] = qb;
    if (a != a) a = __uint_as_float(0x7FC00000u);      // canonical NaN (Java has one NaN value)
    if (b != b) b = __uint_as_float(0x7FC00000u);
    out.idx_local[o] = wloc;
    out.idx_global[o] = gi;
    out.iso[o] = k;
    out.a[o] = a;
    out.b[o] = b;
    out.err[o] = f32_from_orderable((uint32_t)(kk >> 32));
    // the same row once more as one 24-byte record: what a rank contributes to the codebook gather
    int32_t* rec = out.records + 6 * o;
    rec[0] = wloc;
    rec[1] = (int32_t)__float_as_uint(a);
    rec[2] = (int32_t)__float_as_uint(b);
    rec[3] = k;
    rec[4] = qa;
    rec[5] = qb;
}
#endif

int fic_launch_argb_to_gray(const int32_t* argb, uint8_t* gray, size_t npix, hipStream_t s);
int fic_launch_scale(const uint8_t* gray, uint8_t* scaled, const FicGeom& g, hipStream_t s);
int fic_launch_pool(const uint8_t* scaled, uint8_t* pool_pix, FicDomStat* st, uint32_t* var, double* s64,
                    const FicGeom& g, hipStream_t s);
int fic_launch_range(const uint8_t* gray, uint32_t* rng_pix, FicRngStat* rst, const FicGeom& g, hipStream_t s,
                     int with_copies = 1);      // 0: statistics only (the sweep brings its own range store)
int fic_launch_sweep_generic(const FicBuffers& b, const FicGeom& g, int r_begin, int r_count, hipStream_t s);
int fic_launch_sweep_fast(const FicBuffers& b, const FicGeom& g, int tile0, int ntiles, int chunk_len, int nchunks,
                          hipStream_t s);
int fic_launch_finalize(const FicBuffers& b, const FicOutputs& out, const FicGeom& g, int r_begin, int r_count,
                        hipStream_t s, int from_gray = 0);   // 1: recompute the winner's covariance from the image (no rng_pix)
int fic_launch_collage(const FicBuffers& b, const FicOutputs& out, int32_t* collage, const FicGeom& g, hipStream_t s);
int fic_launch_sqrt_probe(double* out, uint32_t first, uint32_t count, hipStream_t s);

// joint-RGB encode (FC:171-219): per-range results, [N_r] each (qrows: [N_r][5], FC:250-254)
struct FicRgbOutputs {
    int32_t* idx_local;
    int32_t* idx_global;
    float* a;
    float* bR;
    float* bG;
    float* bB;
    int32_t* qrows;
    int32_t* iso = nullptr;  // winning isometry [N_r]; NULL: n_iso = 1 (the reference path: the key carries c, no gather)
};
struct FicRgbBuffers {
    int32_t* argb;           // input [H][W]
    int32_t* scaled;         // [H/2][W/2] packed ARGB
    uint16_t* pool_sum;      // [N_d][n]  R+G+B per domain pixel
    float* pool_cf;          // [N_d][n]  greyD_i = pool_sum - msum as exact f32 (full search at B = 4 / 8 only, else NULL)
    FicRgbDomStat* pool_st;  // [N_d]
    int16_t* rng_t;          // [N_r][n]  greyR_i
    FicRgbRngStat* rng_st;   // [N_r]
    unsigned long long* key; // [N_r]
};
// buffers of the matrix-core full search of one image (k_sweep_q<NK, 3>); all NULL = the VALU sweeps
struct FicRgbQ {
    void *poolQ = nullptr, *dflat = nullptr, *rngQ = nullptr, *qst = nullptr, *rngE = nullptr, *theta_g = nullptr, *amax = nullptr;
    int ndtiles = 0, ndtiles_alloc = 0, nct_alloc = 0, tiles_per_chunk = 0, nchunks = 0;
    unsigned long long* stats = nullptr;     // "sweep_stats" = 1: device counters of k_sweep_q<NK, 3> (fic_rgb_ctx_sweep_stats)
};
int fic_launch_rgb_encode(const FicRgbBuffers& b, const FicRgbOutputs& out, int32_t* collage, const FicGeom& g,
                          hipStream_t s, const FicRgbQ* q = nullptr);
int fic_launch_rgbq(const uint16_t* pool_sum, const FicRgbDomStat* pool_st, const int16_t* rng_t, const FicRgbRngStat* rng_st,
                    unsigned long long* key, void* poolQ, void* dflat, void* rngQ, void* qst, void* rngE, void* theta_g, void* amax,
                    const FicGeom& g, int ndtiles, int ndtiles_alloc, int nct_alloc, int tiles_per_chunk, int nchunks, hipStream_t s,
                    unsigned long long* stats = nullptr);

// opt-in matrix-core sweeps ("sweep" = 3)
int fic_mfma8_group(int B);          // range blocks per workgroup of the 8-isometry kernel
int fic_launch_mfma_prep_pool(const uint8_t* pool_pix, void* poolB, const FicGeom& g, int ndtiles_alloc, hipStream_t s);
int fic_launch_mfma_prep_range(const uint32_t* rng_pix, const FicRngStat* rng_st, void* rngA, int* rconst,
                               const FicGeom& g, int ngroups, hipStream_t s);
int fic_launch_sweep_mfma(const FicBuffers& b, const void* poolB, const void* rngA, const int* rconst, const FicGeom& g,
                          int ngroups, int group0, int ngroups_launch, int ndtiles, int ndtiles_alloc, int tiles_per_chunk,
                          int nchunks, hipStream_t s);
int fic_mfma1_ct(int B);
int fic_launch_mfma1_prep(const FicBuffers& b, void* poolA, void* pool_sw, void* rngB, void* rconst, const FicGeom& g,
                          int ndtiles_alloc, int nctiles_alloc, hipStream_t s);
int fic_launch_sweep_mfma1(const FicBuffers& b, const void* poolA, const void* pool_sw, const void* rngB,
                           const void* rconst, const FicGeom& g, int ct_begin, int ct_end, int ndtiles, int ndtiles_alloc,
                           int nctiles_alloc, int tiles_per_chunk, int nchunks, hipStream_t s);
// bf16-operand matrix-core sweeps (fic_bf16.hip): "sweep" = 3 at B = 4 / 8
int fic_bf16_steps(int B);           // MFMA steps of K = 16 per block
int fic_bf16_group8(int B);          // range blocks per workgroup, 8-isometry kernel
int fic_bf16_ct1(int B);             // column tiles (x32 ranges) per workgroup, 1-isometry kernel
int fic_launch_bf16_prep(const FicBuffers& b, void* poolF, void* pool_w, void* rngF, const FicGeom& g, int ndtiles_alloc,
                         int nrtiles_alloc, hipStream_t s);
int fic_launch_sweep_bf16(const FicBuffers& b, const void* poolF, const void* pool_w, const void* rngF, const FicGeom& g,
                          int nrtiles_alloc, int group0, int ngroups_launch, int ndtiles, int ndtiles_alloc, int tiles_per_chunk, int nchunks,
                          hipStream_t s);
int fic_launch_sweep_bf16_1(const FicBuffers& b, const void* poolF, const void* pool_w, const void* rngF, const FicGeom& g,
                            int ct_begin, int ct_end, int ndtiles, int ndtiles_alloc, int nctiles_alloc, int tiles_per_chunk,
                            int nchunks, hipStream_t s);
// VALU sweep with algebraic isometries (fic_d4.hip): n_iso = 8, B = 8 / 16
int fic_d4_words(int B);             // dwords (dot2 pairs) per block in the group-Fourier form, 0 if not built for B
int fic_launch_d4_prep(const FicBuffers& b, uint32_t* rng_d4, uint32_t* pool_d4, const FicGeom& g, hipStream_t s);
int fic_launch_sweep_d4(const FicBuffers& b, const uint32_t* rng_d4, const uint32_t* pool_d4, const FicGeom& g, int tile0,
                        int ntiles, int chunk_len, int nchunks, hipStream_t s);
// default full-search sweep (fic_q.hip, "sweep" = 6): normalised f16 prune GEMM on the matrix cores + exact evaluation of survivors
int fic_q_ct(int B);                 // column tiles (x32 columns) per workgroup
int fic_q_ctw_host(int B);           // column tiles (x32 columns) one wave keeps in registers
int fic_q_prep_fused(const FicGeom& g, int ndtiles_alloc, int ngrp);   // 1: fic_launch_q_prep makes the scaled image itself (no k_scale before it)
int fic_q_shape16(const FicGeom& g);   // 1: k_sweep_q16 (v_mfma_f32_16x16x32_f16) runs this geometry's 1-isometry sweep
int fic_q_multi_kind(int nchunks, int tiles_per_chunk);   // 0: k_sweep_q<.., false>, 1: <.., true>, 2: k_sweep_qs / k_sweep_q16s (short chunks)
int fic_q_cols_per_range(int B, int n_iso);   // sweep columns per range block: 1 (1 isometry), 8 (B = 4), 4 (isometry pairs, B = 8 / 16)
int fic_q_unroll(int B, int n_iso);   // unroll factor of the sweep loop: chunks are whole multiples, the store has that many spare tiles twice
int fic_q_resident(int B);          // workgroups of k_sweep_q a CU holds at once (chunk policy)
int fic_launch_q_prep(const FicBuffers& b, void* poolQ, void* dflat, void* rngQ, void* rngC, void* rngE, void* theta_g,
                      const FicGeom& g, int ndtiles_alloc, int nct_alloc, int grp0, int ngrp, hipStream_t s);
int fic_launch_sweep_q(const FicBuffers& b, const void* poolQ, const void* dflat, const void* rngQ, const void* rngC, const void* rngE,
                       void* theta_g, const FicGeom& g, int ct_begin, int ct_end, int ndtiles, int ndtiles_alloc,
                       int nct_alloc, int tiles_per_chunk, int nchunks, hipStream_t s, unsigned long long* stats = nullptr, int dbg_noflag = 0,
                       const FicOutputs* fin_out = nullptr, unsigned int* fin_count = nullptr, int r_begin = 0, int r_count = 0);
// The prune of the two fast sweeps skips a pair when |C'| <= (int) fl(tau * s32'); tau carries the safety factor 1 - 2^-18 that
// the derivation in fic_lsq.hip needs.  Option "lsq_tau_widen" = k in 8..24 multiplies tau by 1 + 2^-k after it: diagnostic,
// > 0 gives WRONG codebooks (the bound tests use it to show that their inputs catch a bound that is too wide); 0: times 1.
#define FIC_LSQ_TAU_SAFETY 0.99999618530273437500f
inline float fic_lsq_tau_widen(int k) { return k > 0 ? 1.0f + (float)(1.0 / (double)(1ll << k)) : 1.0f; }
// least-squares domain search (fic_lsq.hip, option "search" = 1).  Its stores, beside FicBuffers:
//   pool  : u32x4 [planes][Nd_pad]          {S_d, S_dd, V = n S_dd - S_d^2, bits of (float) sqrt((double) V)}
//   rng   : u32x2 [planes][Nr_pad]          {S_r, S_rr}
//   slotE : i64   [planes][nslots][Nr_pad]  smallest E of one (pool chunk, isometry group) of the sweep, and in
//   slotC : u32   [planes][nslots][Nr_pad]  its candidate c = wloc * n_iso + k     (the generic sweep: one slot)
//   E     : i64   [planes][Nr]              the winner's E (fic_ctx_get_lsq_error_host)
struct FicLsq {
    void* pool;
    void* rng;
    void* slotE;
    uint32_t* slotC;
    void* E;
};
int fic_lsq_slots(const FicGeom& g, int nchunks);   // slots of a fast sweep over nchunks pool chunks
int fic_launch_lsq_stat(const FicBuffers& b, const FicLsq& q, const FicGeom& g, hipStream_t s);
int fic_launch_sweep_lsq_generic(const FicBuffers& b, const FicLsq& q, const FicGeom& g, int r_begin, int r_count, hipStream_t s);
int fic_launch_sweep_lsq_fast(const FicBuffers& b, const FicLsq& q, const FicGeom& g, int tile0, int ntiles, int chunk_len, int nchunks,
                              hipStream_t s, unsigned long long* stats = nullptr,    // stats u64 [8]: "sweep_stats" counters or NULL
                              int tau_widen = 0);                                     // option "lsq_tau_widen"
int fic_launch_finalize_lsq(const FicBuffers& b, const FicOutputs& out, const FicLsq& q, int nslots, const FicGeom& g, int r_begin,
                            int r_count, hipStream_t s);
// The same search on the matrix cores (fic_lsq_q.hip, context option "lsq_engine" = 1): a normalised f16 prune
// GEMM decides which pairs can be skipped, the others are evaluated as above.  Its stores, beside FicBuffers and FicLsq
// (NK = n / 16; a fragment is 64 lanes x 8 f16, laid out as fic_q.hip's frag_slot for v_mfma_f32_32x32x16_f16):
//   poolQ : f16 [planes][ndtiles][NK][64][8]     A fragments, 32 pool blocks per domain tile (rows past N_d and flat blocks: zeros)
//   rngQ  : f16 [planes][nct_alloc][NK][64][8]   B fragments, 32 columns per column tile, column = range block * n_iso + isometry
//   rngE  : f32 [planes][Nr_pad]                 the rounding allowance Er of the prune test
//   rngR  : u32 [planes][Nr_pad]                 R = n S_rr - S_r^2
struct FicLsqQ {
    void* poolQ = nullptr;
    void* rngQ = nullptr;
    void* rngE = nullptr;
    void* rngR = nullptr;
    int ndtiles = 0, nct_alloc = 0;
};
int fic_lsq_q_ct(int B);            // column tiles (x32 columns) per workgroup of k_sweep_lsq_q
int fic_launch_lsq_q_prep(const FicBuffers& b, const FicLsq& q, const FicLsqQ& s, const FicGeom& g, int eshift, hipStream_t st);
// column tiles [ct_begin, ct_end); nchunks pool chunks of tiles_per_chunk domain tiles, none empty and none longer than
// fic_lsq_q_max_tiles_per_chunk (fic_lsq_q_chunks.h); slots per plane = nchunks
int fic_launch_sweep_lsq_q(const FicBuffers& b, const FicLsq& q, const FicLsqQ& s, const FicGeom& g, int ct_begin, int ct_end,
                           int tiles_per_chunk, int nchunks, hipStream_t st, unsigned long long* stats = nullptr,
                           int tau_widen = 0);
// least-squares domain search of the joint-RGB path (fic_lsq_rgb.hip, option "search" = 1 of a colour context).
// Its stores (Nr_pad = N_r rounded up to whole tiles of 64 range blocks):
//   pool3   : u8    [planes][Nd_pad][3][n]               pool blocks, planar R, G, B (tail zeroed)
//   pool_st : u32x8 [planes][Nd_pad]                     {S_d R, G, B, S_dd, V, bits of (float) sqrt((double) V), 0, 0}
//   rng3    : u32   [planes][tiles][n_iso][3 DW][64]     lane-transposed isometry copies of the range blocks, planar
//   rng_st  : u32x4 [planes][Nr_pad]                     {S_r R, G, B, S_rr}
//   slotE   : i64   [planes][nslots][Nr_pad]             smallest E of one (pool chunk, isometry group) of the sweep, and in
//   slotC   : u32   [planes][nslots][Nr_pad]             its candidate c = wloc * n_iso + k     (the generic sweep: one slot)
//   E       : i64   [planes][Nr]                         the winner's E (fic_rgb_ctx_get_lsq_error_host)
struct FicLsqRgb {
    void* pool3 = nullptr;
    void* pool_st = nullptr;
    void* rng3 = nullptr;
    void* rng_st = nullptr;
    void* slotE = nullptr;
    uint32_t* slotC = nullptr;
    void* E = nullptr;
    int Nr_pad = 0;
};
int fic_lsq_rgb_variant(int B, int n_iso, int* NC);     // 0 and the isometries per workgroup of k_sweep_lsq_rgb_fast, or -1: none
int fic_lsq_rgb_slots(const FicGeom& g, int nchunks);   // slots of a fast sweep over nchunks pool chunks
int fic_launch_lsq_rgb_prep(const int32_t* argb, const int32_t* scaled, const FicLsqRgb& q, const FicGeom& g, hipStream_t s);
int fic_launch_sweep_lsq_rgb_generic(const FicLsqRgb& q, const FicGeom& g, hipStream_t s);
int fic_launch_sweep_lsq_rgb_fast(const FicLsqRgb& q, const FicGeom& g, int chunk_len, int nchunks, hipStream_t s,
                                  unsigned long long* stats = nullptr,    // stats u64 [8]: "sweep_stats" counters or NULL
                                  int tau_widen = 0);                      // option "lsq_tau_widen"
int fic_launch_finalize_lsq_rgb(const FicRgbOutputs& out, const FicLsqRgb& q, int nslots, const FicGeom& g, hipStream_t s);
// The same search on the matrix cores (fic_lsq_rgb_q.hip, colour context option "lsq_engine" = 1), B = 4 / 8 /
// 16: a block is one vector of 3 n entries (planar), NK = 3 n / 16.  Its stores, beside FicLsqRgb (fragments as in FicLsqQ):
//   poolQ : f16 [planes][ndtiles][NK][64][8]   A fragments, 32 pool blocks per domain tile (rows past N_d and V == 0: zeros)
//   rngQ  : f16 [planes][nct][NK][64][8]       B fragments, 32 columns per column tile, column = range block * n_iso + isometry
//   rngE  : f32 [planes][Nr_pad]               the rounding allowance Er of the prune test
//   rngR  : u32 [planes][Nr_pad]               R = n S_rr - sum_ch S_r^2 (unsigned: < 2^31.6 at B = 16)
struct FicLsqRgbQ {
    void* poolQ = nullptr;
    void* rngQ = nullptr;
    void* rngE = nullptr;
    void* rngR = nullptr;
    int ndtiles = 0, nct = 0;
};
int fic_launch_lsq_rgb_q_prep(const FicLsqRgb& q, const FicLsqRgbQ& s, const FicGeom& g, int eshift, hipStream_t st);
// nchunks pool chunks of tiles_per_chunk domain tiles, none empty (fic_lsq_q_chunks.h); slots per plane = nchunks
int fic_launch_sweep_lsq_rgb_q(const FicLsqRgb& q, const FicLsqRgbQ& s, const FicGeom& g, int tiles_per_chunk, int nchunks,
                               hipStream_t st, unsigned long long* stats = nullptr, int tau_widen = 0);
// stages of fic_launch_rgb_encode on their own, over g.planes images: scaleImageRGB and the collage of the rows in `out`
int fic_launch_scale_rgb_planes(const int32_t* argb, int32_t* scaled, const FicGeom& g, hipStream_t s);
int fic_launch_rgb_collage(const int32_t* scaled, const FicRgbOutputs& out, int32_t* collage, const FicGeom& g, hipStream_t s);
int fic_launch_decode_iteration_rgb(int32_t* scaled, int32_t* image, const int32_t* qrows5, FicDecodeState* state,
                                    uint32_t* sqbuf, int counter, const FicGeom& g, hipStream_t s,
                                    const int32_t* iso = nullptr);   // iso [N_r]: an n_iso = 8 codebook of a context, NULL: identity
int fic_launch_scale_rgb(const int32_t* argb, int32_t* scaled, const FicGeom& g, hipStream_t s);   // one image

// decoder (FC:356-421)
// maps: fic_float_sum_map_words(count) u32 of scratch; out2[0] = the sum, out2[1] = segments that took the sequential-order path
int fic_launch_float_sum_probe(float carry, const uint32_t* vals, int count, uint32_t* maps, float* out2, hipStream_t s);
size_t fic_float_sum_map_words(size_t count);
// u32 words of the decoder's `sqbuf` scratch for `planes` images of wh pixels (squares + segment maps of the float sum)
size_t fic_decode_sq_words(size_t planes, size_t wh);
// sqbuf: u32 [planes][W*H] per-pixel squared changes of the iteration in Java's visiting order (for the sequential f32 sum)
int fic_launch_decode_step(FicDecodeState* state, uint32_t* sqbuf, int counter, int wh, int planes, hipStream_t s);
int fic_launch_decode_iteration(uint8_t* scaled, uint8_t* image, const int32_t* qrows, const int32_t* iso,
                                FicDecodeState* state, uint32_t* sqbuf, int counter, const FicGeom& g, hipStream_t s);

// quadtree codec (fic_quadtree.hip), grey and joint RGB.  The pixel format of an image and its quantised rows:
//   QtGrey    bytes,       rows {idx_local, qa, qb} + an isometry column  -> leaf rows [7] {x, y, B, idx_local, qa, qb, iso}
//   QtRgb     packed ARGB, rows {idx_local, q1, q2, q3, q4}               -> leaf rows [8] {x, y, B, idx_local, q1, q2, q3, q4}
//   QtRgbIso  packed ARGB, the same rows + an isometry column (4.17)      -> leaf rows [9] {x, y, B, idx_local, q1, q2, q3, q4, iso}
// One leaf of the decoder's per-level lists: position, global domain block (the level's window_to_global), offset of its B*B
// squares in `sqbuf` (prefix sum of B^2 over the leaves before it), quantised row: {qa, qb, iso, 0} grey, {q1, q2, q3, q4} colour.
struct FicQtLeaf {
    int32_t x, y, gi, sqoff, q[4];
};
// The same with the isometry beside the full colour row (QtRgbIso only: the two older formats keep their 32-byte leaf)
struct FicQtLeafIso {
    int32_t x, y, gi, sqoff, q[4], k;
};
struct QtGrey {
    using Px = uint8_t;
    using Leaf = FicQtLeaf;
    static constexpr int QW = 3;             // ints per quantised row
    static constexpr bool kIso = true;       // an isometry column beside the rows (NULL: n_iso = 1, iso 0)
    static constexpr int kLeafInts = 3 + QW + 1;
};
struct QtRgb {
    using Px = int32_t;
    using Leaf = FicQtLeaf;
    static constexpr int QW = 5;
    static constexpr bool kIso = false;
    static constexpr int kLeafInts = 3 + QW;
};
struct QtRgbIso {
    using Px = int32_t;
    using Leaf = FicQtLeafIso;
    static constexpr int QW = 5;
    static constexpr bool kIso = true;
    static constexpr int kLeafInts = 3 + QW + 1;
};
// The batch of planes behind the launchers below (the one-shot entries run the batch of one plane).  The plane is
// a grid dimension of every kernel and no workgroup spans two planes.  Every array gets the plane as its slowest index: image
// [planes][H][W], scaled [planes][Hs][Ws], qrows [planes][Nr_l][QW], iso [planes][Nr_l], keys / gains [planes][nkeys], top_sum
// [planes], counts [planes][Ntop], offs [planes][Ntop + 1], stats [planes][4], the select areas [planes][FIC_QT_SELECT(_W)_WORDS];
// the SSE of level l starts at the pointer given for it and plane p's sse_stride u32 further; the leaves of plane p leaf_stride
// ints behind those of plane 0.  The rules' parameters are read from device memory: the threshold of plane p is the float in
// param[p], lambda is param[p] (the pointer handed to the _rd launchers), the selects take ranks[p] / values[p] and leave
// their result in param[p] as well.
struct FicQtPlanes {
    int planes;
    int Nr[3];               // range blocks per plane of every level
    int nkeys;               // Ntop + n1
    size_t sse_stride;       // u32
    size_t leaf_stride;      // ints
    int* n_leaves;           // [planes]: the leaf counts once more (also offs[p][Ntop])
    uint32_t* param;         // [planes]
    const uint32_t* ranks;   // [planes]: fic_launch_qt_select
    const long long* values; // [planes]: fic_launch_qt_select_w
};
// sse u32 [g.Nr] per plane: collage SSE (colour: over the three channels) of every range block of one level from its quantised
// rows [N_r][Fmt::QW]; image the original [H][W], scaled its 2:1 copy [Hs][Ws] (k_scale / scaleImageRGB); iso: formats with kIso only
template <typename Fmt>
int fic_launch_leaf_sse(const typename Fmt::Px* image, const typename Fmt::Px* scaled, const int32_t* qrows, const int32_t* iso,
                        uint32_t* sse, const FicGeom& g, hipStream_t s, const FicQtPlanes& P);
// split + compaction over nl levels (B_max >> l) under the thresholds in P.param: counts int [Ntop], offs int [Ntop + 1]
// (offs[Ntop] = leaves), leaves int32 [leaves][Fmt::kLeafInts] (NULL: count only); room for the largest possible count is the
// caller's.  iso: formats with kIso only
template <typename Fmt>
int fic_launch_qt_compact(const uint32_t* const* sse, const int32_t* const* qrows, const int32_t* const* iso, const int* Rw,
                          int nl, int B_max, int Rw_top, int Ntop, int* counts, int* offs, int32_t* leaves, hipStream_t s,
                          const FicQtPlanes& P);
// Encode to a leaf budget, on the same per-level SSE arrays.  keys u32 [Ntop + n1]: the split key e(v) of every
// block above B_min, level 0 first; n1 = N_r of level 1 with three levels, else 0.
int fic_launch_qt_keys(const uint32_t* const* sse, const int* Rw, int nl, int B_max, int Rw_top, int Ntop, int n1, uint32_t* keys,
                       hipStream_t s, const FicQtPlanes& P);
// Radix select over n < 2^31 keys: work u32 [FIC_QT_SELECT_WORDS] = four 256-bin histograms, then {K, bits of the threshold,
// #{keys > K}, 0}, K the key of rank P.ranks[p] <= n in descending order (0 past the last key), the threshold the smallest float
// >= K / 256; P.param[p] = word `param_word` of plane p's result (0: K, 1: the threshold's bits)
constexpr int FIC_QT_SELECT_WORDS = 4 * 256 + 4;
int fic_launch_qt_select(const uint32_t* keys, uint32_t n, uint32_t* work, hipStream_t s, const FicQtPlanes& P, int param_word);
// stats u64 [4] = {collage SSE of the leaves, leaves of side B_max, B_max / 2, B_max / 4} of the tree under the thresholds in P.param
int fic_launch_qt_tree_stats(const uint32_t* const* sse, const int* Rw, int nl, int B_max, int Rw_top, int Ntop,
                             unsigned long long* stats, hipStream_t s, const FicQtPlanes& P);
// Encode by rate-distortion pruning, on the same per-level SSE arrays.  keys u32 / gains i64 [Ntop + n1]: e(v)
// and G_v of every block above B_min in the order of fic_launch_qt_keys; *top_sum = the sum of the SSE of the top-level blocks.
int fic_launch_qt_rd_keys(const uint32_t* const* sse, const int* Rw, int nl, int B_max, int Rw_top, int Ntop, int n1, uint32_t* keys,
                          long long* gains, unsigned long long* top_sum, hipStream_t s, const FicQtPlanes& P);
// Weighted radix select over n < 2^31 (key, gain) pairs: work u64 [FIC_QT_SELECT_W_WORDS] = four 256-bin gain sums, then {b in the
// low 32 bits, #{keys > b}, their summed gain, 0}: b the largest of the keys and 0 with sum_{key > b} gain >= need, 0 when there is
// none, and P.param[p] = b; need = (int64) total[p] - P.values[p], both on the device.  The cumulated gain over descending
// distinct keys must not fall.
constexpr int FIC_QT_SELECT_W_WORDS = 4 * 256 + 4;
int fic_launch_qt_select_w(const uint32_t* keys, const long long* gains, uint32_t n, const unsigned long long* total,
                           unsigned long long* work, hipStream_t s, const FicQtPlanes& P);
// fic_launch_qt_compact / _tree_stats with the split rule "e(v) > lambda[p]": keys as fic_launch_qt_rd_keys writes them, lambda a
// device pointer (where a select left it)
template <typename Fmt>
int fic_launch_qt_compact_rd(const uint32_t* const* sse, const int32_t* const* qrows, const int32_t* const* iso, const int* Rw,
                             int nl, int B_max, int Rw_top, int Ntop, const uint32_t* keys, const uint32_t* lambda, int* counts,
                             int* offs, int32_t* leaves, hipStream_t s, const FicQtPlanes& P);
int fic_launch_qt_tree_stats_rd(const uint32_t* const* sse, const int* Rw, int nl, int B_max, int Rw_top, int Ntop, const uint32_t* keys,
                                const uint32_t* lambda, unsigned long long* stats, hipStream_t s, const FicQtPlanes& P);
// one paint (decodeGreyScale / decodeRGB) of the n leaves of side g.B (one plane; g = that level's geometry)
template <typename Fmt>
int fic_launch_decode_paint_leaves(const typename Fmt::Px* scaled, typename Fmt::Px* image, const typename Fmt::Leaf* lv, int n,
                                   FicDecodeState* state, uint32_t* sqbuf, int counter, const FicGeom& g, hipStream_t s);
// Decode and collage of a batch from the encoder's leaf table on the device (QtGrey and QtRgbIso, the batched
// handle's formats).  What the two kernels know of the context: its levels at the decode's zoom (the same block counts, sides
// and image times zoom: make_decode_geometry) and the ladder and image of the encode.
struct FicQtDecode {
    FicGeom g[3];
    int nl, zoom;
    int B_max, B_min, W, H;  // of the encode
    int Rw_top, Rw_min, Nr_min, n_iso;
    size_t leaf_stride;      // ints between the tables of two planes
};
// Checks and resolves the table of every plane: entries int32 [planes][Nr_min][kQtEntryInts], cells int32 [planes][Nr_min], cover
// int32 [planes] (fic_qt_decode_plan.h); a plane whose table is not a valid tiling gets state[p].bad_index here or in the paint.
// state [planes] must hold the loop's initial state (bad_index 0) on s before this.
template <typename Fmt>
int fic_launch_qt_resolve(const int32_t* leaves, const int* n_leaves, const FicQtDecode& D, int planes, int32_t* entries, int32_t* cells,
                          int32_t* cover, FicDecodeState* state, hipStream_t s);
// One paint of all leaves of all planes from scaled [planes][zH / 2][zW / 2] into image [planes][zH][zW]; collage: scaled is the
// input's 2:1 copy, the paint runs once, sqbuf and counter are not used.
template <typename Fmt>
int fic_launch_qt_paint_planes(const typename Fmt::Px* scaled, typename Fmt::Px* image, const int32_t* entries, const int32_t* cells,
                               const int32_t* cover, FicDecodeState* state, uint32_t* sqbuf, int counter, bool collage, const FicQtDecode& D,
                               int planes, hipStream_t s);
