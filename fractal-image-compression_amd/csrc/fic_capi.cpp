// fic_capi.cpp -- C ABI (include/fic.h) over the gfx950 kernels.  Host-side orchestration only:
// validation, device buffers, launch order, result copies.  No compute happens on the CPU and
// there is no CPU fallback: without a HIP device every compute entry returns FIC_E_NO_DEVICE.
// (decoder entries: fic_capi_decode.cpp; joint-RGB contexts: fic_capi_rgb.cpp; multi-device entry: fic_capi_multi.cpp;
// error state, geometry and every stream writer / parser: fic_stream.cpp)
#include "fic_internal.h"
#include "fic_lsq_q_chunks.h"
#include "fic_sweep_chunks.h"

namespace ficd {

int check_device(int device)
{
    int ndev = fic_device_count();
    if (ndev <= 0 || device < 0 || device >= ndev) return fail(FIC_E_NO_DEVICE, "no HIP device %d (this library has no CPU path)", device);
    HIP_TRY(hipSetDevice(device));
    return FIC_OK;
}

bool create_device_ok(int device)
{
    int ndev = fic_device_count();
    if (ndev <= 0) { fail(FIC_E_NO_DEVICE, "no HIP device visible (this library has no CPU path)"); return false; }
    if (device < 0 || device >= ndev) { fail(FIC_E_NO_DEVICE, "device %d out of range (0..%d)", device, ndev - 1); return false; }
    if (hipSetDevice(device) != hipSuccess) { fail(FIC_E_HIP, "hipSetDevice(%d) failed", device); return false; }
    return true;
}

IdleCache<fic_ctx, 16> g_idle_grey;

}  // namespace ficd

using namespace ficd;

fic_ctx::~fic_ctx()
{
    if (!own_stream) return;
    (void)hipSetDevice(device);
    (void)hipStreamDestroy(own_stream);
}

namespace {

// ---- sweep orchestration helpers (used by fic_ctx_encode); the pool-chunk rules are fic_sweep_chunks.h's --------------------

// VALU sweep k_sweep_fast ("sweep" = 2) over tiles [tile0, tile0 + ntiles).
int valu_sweep(fic_ctx* c, int tile0, int ntiles, hipStream_t s, int* nchunks_out)
{
    const FicGeom& g = c->g;
    int NR, NC;
    fic_fast_variant(g.B, g.n_iso, &NR, &NC);
    const SweepChunks k = valu_chunks(g.Nd, (long long)ntiles * (g.n_iso / NC) * g.planes, c->opt_chunks, FIC_VALU_CHUNK_TARGET, true);
    if (fic_launch_sweep_fast(c->b, g, tile0, ntiles, k.len, k.nchunks, s)) return fail(FIC_E_HIP, "k_sweep_fast launch failed");
    *nchunks_out = k.nchunks;
    return FIC_OK;
}

// VALU sweep for n_iso = 8 with the isometries taken algebraically (k_sweep_d4, fic_d4.hip): slot prep + sweep.
int d4_available(const FicGeom& g) { return g.full && g.n_iso == 8 && g.NR == 1 && fic_d4_words(g.B) > 0; }
int d4_prep(fic_ctx* c, hipStream_t s)
{
    const FicGeom& g = c->g;
    const size_t NW = (size_t)fic_d4_words(g.B), P = (size_t)g.planes;
    int rc = c->mem.ensure(c->d4_rng, P * g.tiles * NW * 64);
    if (rc == FIC_OK) rc = c->mem.ensure(c->d4_pool, P * g.Nd_pad * NW);
    if (rc) return rc;
    if (fic_launch_d4_prep(c->b, c->d4_rng, c->d4_pool, g, s)) return fail(FIC_E_HIP, "k_range_d4 / k_pool_d4 launch failed");
    return FIC_OK;
}
int d4_sweep(fic_ctx* c, int tile0, int ntiles, hipStream_t s, int* nchunks_out)
{
    const FicGeom& g = c->g;
    const SweepChunks k = valu_chunks(g.Nd, (long long)ntiles * g.planes, c->opt_chunks, FIC_VALU_CHUNK_TARGET, false);
    if (fic_launch_sweep_d4(c->b, c->d4_rng, c->d4_pool, g, tile0, ntiles, k.len, k.nchunks, s))
        return fail(FIC_E_HIP, "k_sweep_d4 launch failed");
    *nchunks_out = k.nchunks;
    return FIC_OK;
}

// The exact-covariance matrix-core sweeps of round 1 ("sweep" = 3 / 4, fic_bf16.hip / fic_mfma.hip) lose to k_sweep_q everywhere; they are
// kept as independent cross-checks for the test-suite (a third and fourth implementation of the same search) and are compiled
// only into builds with FIC_BUILD_XCHECK (build.py: on by default, FIC_BUILD_XCHECK=0 for a deployment build).
#ifdef FIC_BUILD_XCHECK
// Opt-in matrix-core sweeps: geometry of the fragment stores.
struct MatrixCoreShape {
    bool iso8;
    bool bf16;                       // bf16 operands (B = 4 / 8, B = 16 with 8 isometries; never with "sweep" = 4), else i8
    int steps;                       // MFMA steps per block: K = 16 (bf16) or K = 32 (i8)
    int ndtiles, ndtiles_alloc;      // domain tiles (x32 blocks), + 1 spare for the prefetch
    int nctiles_alloc;               // n_iso = 1: column tiles (x32 ranges), padded for the last workgroup
    int G8, ngroups8;                // n_iso = 8: range blocks per workgroup, number of groups
    int ct1;                         // n_iso = 1: column tiles per workgroup
};
MatrixCoreShape matrix_core_shape(const FicGeom& g, int kind)
{
    MatrixCoreShape m;
    m.iso8 = g.n_iso == 8;
    // bf16 operands wherever they are faster: B = 4/8, and B = 16 with 8 isometries (51 vs 79 ms at 4096x4096; with
    // 1 isometry the i8 kernel wins there, 8.6 vs 9.2 ms)
    m.bf16 = kind == 3 && (g.B <= 8 || g.n_iso == 8);
    m.steps = m.bf16 ? fic_bf16_steps(g.B) : (g.n <= 32 ? 1 : g.n / 32);
    m.ndtiles = (g.Nd + 31) / 32;
    m.ndtiles_alloc = m.ndtiles + 1;
    m.nctiles_alloc = g.Nr_pad / 32 + 32;
    m.G8 = m.bf16 ? fic_bf16_group8(g.B) : fic_mfma8_group(g.B);
    m.ngroups8 = (g.Nr_pad + m.G8 - 1) / m.G8;
    m.ct1 = m.bf16 ? fic_bf16_ct1(g.B) : fic_mfma1_ct(g.B);
    return m;
}
int matrix_core_prep(fic_ctx* c, int kind, hipStream_t s)
{
    const FicGeom& g = c->g;
    const MatrixCoreShape m = matrix_core_shape(g, kind);
    const size_t P = (size_t)g.planes;
    if ((c->mfma_poolB || c->mfma_rngA || c->mfma_sw || c->mfma_rconst) && c->mfma_bf16 != (int)m.bf16) {     // operand type changed ("sweep" 3 <-> 4): new fragment stores
        HIP_TRY(hipStreamSynchronize(s));
        c->mem.release(c->mfma_poolB);
        c->mem.release(c->mfma_rngA);
        c->mem.release(c->mfma_sw);
        c->mem.release(c->mfma_rconst);
    }
    {
        // every store is ensured on its own pointer: a failed allocation leaves the others usable and is retried next time
        c->mfma_bf16 = (int)m.bf16;
        const size_t rtiles = m.iso8 ? (size_t)m.ngroups8 * (m.G8 / 4) : (size_t)m.nctiles_alloc;   // 32-row/column range tiles
        int rc = c->mem.ensure(c->mfma_poolB, P * m.ndtiles_alloc * m.steps * 64 * 16);
        if (rc == FIC_OK) rc = c->mem.ensure(c->mfma_rngA, P * rtiles * m.steps * 64 * 16);
        if (rc == FIC_OK) rc = c->mem.ensure(c->mfma_sw, P * m.ndtiles_alloc * 32 * 8);
        if (rc == FIC_OK && !m.bf16) rc = c->mem.ensure(c->mfma_rconst, m.iso8 ? P * rtiles * 16 : P * rtiles * 32 * 16 / sizeof(int));
        if (rc) return rc;
    }
    if (m.bf16) {
        const int rtiles = m.iso8 ? m.ngroups8 * (m.G8 / 4) : m.nctiles_alloc;
        if (fic_launch_bf16_prep(c->b, c->mfma_poolB, c->mfma_sw, c->mfma_rngA, g, m.ndtiles_alloc, rtiles, s))
            return fail(FIC_E_HIP, "bf16 fragment prep launch failed");
    } else if (m.iso8) {
        if (fic_launch_mfma_prep_pool(c->b.pool_pix, c->mfma_poolB, g, m.ndtiles_alloc, s) ||
            fic_launch_mfma_prep_range(c->b.rng_pix, c->b.rng_st, c->mfma_rngA, c->mfma_rconst, g, m.ngroups8, s))
            return fail(FIC_E_HIP, "mfma prep launch failed");
    } else if (fic_launch_mfma1_prep(c->b, c->mfma_poolB, c->mfma_sw, c->mfma_rngA, c->mfma_rconst, g, m.ndtiles_alloc,
                                     m.nctiles_alloc, s)) {
        return fail(FIC_E_HIP, "mfma1 prep launch failed");
    }
    return FIC_OK;
}
int matrix_core_sweep(fic_ctx* c, int kind, int tile0, int tile1, hipStream_t s, int* nchunks_out)
{
    const FicGeom& g = c->g;
    const MatrixCoreShape m = matrix_core_shape(g, kind);
    const int tsz = 64 * g.NR;
    const long long ranges = (long long)(tile1 - tile0) * tsz, per_wg = m.iso8 ? m.G8 : 32LL * m.ct1;
    const SweepChunks k = xcheck_chunks(m.ndtiles, (ranges + per_wg - 1) / per_wg * g.planes, c->opt_chunks);
    const int tiles_per_chunk = k.len, nchunks = k.nchunks;
    if (m.iso8) {
        const int g0 = (tile0 * tsz) / m.G8, g1 = (tile1 * tsz + m.G8 - 1) / m.G8;   // groups covering the tile span
        const int rc = m.bf16 ? fic_launch_sweep_bf16(c->b, c->mfma_poolB, c->mfma_sw, c->mfma_rngA, g, m.ngroups8 * (m.G8 / 4), g0,
                                                      g1 - g0, m.ndtiles, m.ndtiles_alloc, tiles_per_chunk, nchunks, s)
                              : fic_launch_sweep_mfma(c->b, c->mfma_poolB, c->mfma_rngA, c->mfma_rconst, g, m.ngroups8, g0,
                                                      g1 - g0, m.ndtiles, m.ndtiles_alloc, tiles_per_chunk, nchunks, s);
        if (rc) return fail(FIC_E_HIP, "8-isometry matrix-core sweep launch failed");
    } else {
        const int ct_begin = tile0 * (tsz / 32), ct_end = tile1 * (tsz / 32);
        const int rc = m.bf16 ? fic_launch_sweep_bf16_1(c->b, c->mfma_poolB, c->mfma_sw, c->mfma_rngA, g, ct_begin, ct_end,
                                                        m.ndtiles, m.ndtiles_alloc, m.nctiles_alloc, tiles_per_chunk, nchunks, s)
                              : fic_launch_sweep_mfma1(c->b, c->mfma_poolB, c->mfma_sw, c->mfma_rngA, c->mfma_rconst, g, ct_begin,
                                                       ct_end, m.ndtiles, m.ndtiles_alloc, m.nctiles_alloc, tiles_per_chunk,
                                                       nchunks, s);
        if (rc) return fail(FIC_E_HIP, "1-isometry matrix-core sweep launch failed");
    }
    *nchunks_out = nchunks;
    return FIC_OK;
}

#else
int matrix_core_prep(fic_ctx*, int, hipStream_t) { return fail(FIC_E_ARGUMENT, "sweep 3 / 4 (cross-check kernels) are not in this build (FIC_BUILD_XCHECK=0)"); }
int matrix_core_sweep(fic_ctx*, int, int, int, hipStream_t, int*) { return fail(FIC_E_ARGUMENT, "sweep 3 / 4 (cross-check kernels) are not in this build (FIC_BUILD_XCHECK=0)"); }
#endif
// Default full-search sweep (fic_q.hip): shapes of its stores, fused prep (pool build + range prep + fragments), launch.
struct QShape {
    int ndtiles, ndtiles_alloc;      // domain tiles (x32 blocks), + zero tiles for the unrolled loop's overrun and prefetch
    int unroll;                      // unroll factor of the sweep loop
    int CT;                          // column tiles (x32 range copies) per workgroup
    int nct_alloc;                   // column tiles allocated (padded for the last workgroup)
};
QShape q_shape(const FicGeom& g)
{
    QShape q;
    q.ndtiles = (g.Nd + 31) / 32;
    q.unroll = fic_q_unroll(g.B, g.n_iso);
    q.ndtiles_alloc = q.ndtiles + 2 * q.unroll;
    q.CT = fic_q_ct(g.B);
    const int nct = g.Nr_pad * fic_q_cols_per_range(g.B, g.n_iso) / 32;
    q.nct_alloc = (nct + q.CT - 1) / q.CT * q.CT + q.CT;
    return q;
}
int q_prep(fic_ctx* c, int tile0, int tile1, hipStream_t s)
{
    const FicGeom& g = c->g;
    const QShape q = q_shape(g);
    const size_t P = (size_t)g.planes, NK = (size_t)g.n / 16;
    DevMem& m = c->mem;
    int rc = m.ensure(c->q_pool, P * q.ndtiles_alloc * NK * 64 * 16);
    if (rc == FIC_OK) rc = m.ensure(c->q_flat, P * q.ndtiles_alloc * sizeof(uint32_t));
    // zeroed once: column tiles past the last range group stay zero fragments
    if (rc == FIC_OK) rc = m.ensure_zeroed(c->q_rng, P * q.nct_alloc * NK * 64 * 16, s);
    if (rc == FIC_OK) rc = m.ensure(c->q_rngC, P * g.Nr_pad * fic_q_cols_per_range(g.B, g.n_iso) * g.n);
    if (rc == FIC_OK) rc = m.ensure(c->q_E, P * g.Nr_pad * sizeof(float));
    // (+ the padded column tiles behind the last plane: the sweep's fast path reads theta_g of every column it owns)
    if (rc == FIC_OK) rc = m.ensure(c->q_thg, (P * g.Nr_pad + (size_t)2 * q.CT * 32 + 64) * sizeof(uint32_t));
    if (rc) return rc;
    const int tsz = 64 * g.NR;
    const int grp0 = tile0 * tsz / 64, grp1 = tile1 * tsz / 64;      // 64-range groups covering the span
    if (fic_launch_q_prep(c->b, c->q_pool, c->q_flat, c->q_rng, c->q_rngC, c->q_E, c->q_thg, g, q.ndtiles_alloc, q.nct_alloc, grp0, grp1 - grp0, s))
        return fail(FIC_E_HIP, "k_pool_q / k_range_q launch failed");
    return FIC_OK;
}
int q_sweep(fic_ctx* c, int tile0, int tile1, hipStream_t s, int* nchunks_out, bool fused_fin = false, int r_begin = 0, int r_count = 0)
{
    const FicGeom& g = c->g;
    const QShape q = q_shape(g);
    const int tsz = 64 * g.NR;
    const int cpr = fic_q_cols_per_range(g.B, g.n_iso);
    const int ct_begin = tile0 * tsz * cpr / 32, ct_end = tile1 * tsz * cpr / 32;
    const SweepChunks k = q_chunks(q.ndtiles, (long long)((ct_end - ct_begin + q.CT - 1) / q.CT) * g.planes, 256LL * fic_q_resident(g.B),
                                   q_min_tiles_grey(g.n_iso), q.unroll, c->opt_chunks);
    const int tiles_per_chunk = k.len, nchunks = k.nchunks;
    if (fused_fin) {                                   // one counter per (plane, column group); the sweep leaves them at zero
        const int rc = c->mem.ensure_zeroed(c->q_fin, (size_t)g.planes * (q.nct_alloc / q.CT + 1), s);
        if (rc) return rc;
    }
    if (fic_launch_sweep_q(c->b, c->q_pool, c->q_flat, c->q_rng, c->q_rngC, c->q_E, c->q_thg, g, ct_begin, ct_end, q.ndtiles, q.ndtiles_alloc,
                           q.nct_alloc, tiles_per_chunk, nchunks, s, c->sweep_stats, c->opt_noflag, fused_fin ? &c->o : nullptr, c->q_fin,
                           r_begin, r_count))
        return fail(FIC_E_HIP, "k_sweep_q launch failed");
    *nchunks_out = nchunks;
    c->last_tiles_per_chunk = tiles_per_chunk;
    return FIC_OK;
}

// Least-squares search ("search" = 1, fic_lsq.hip) of the span: pool build and range prep as for the VALU
// sweeps, the extra sums, k_sweep_lsq_generic (windows, "sweep" = 1) or k_sweep_lsq_fast (full search), k_finalize_lsq.
// Under "lsq_engine" = 1 the matrix-core sweep k_sweep_lsq_q (fic_lsq_q.hip; reported as sweep kind 7) runs
// wherever k_sweep_lsq_fast would.
int lsq_encode(fic_ctx* c, int range_begin, int range_count, hipStream_t s)
{
    const FicGeom& g = c->g;
    int kind = c->opt_sweep;
    if (kind < 0 || kind > 2) return fail(FIC_E_ARGUMENT, "least-squares search: sweep must be 0 (auto), 1 (generic) or 2 (fast), not %d", kind);
    if (kind == 0) kind = g.full ? 2 : 1;
    if (kind == 2 && !g.full) return fail(FIC_E_ARGUMENT, "fast sweep needs full search (wK == Dw == Dh)");
    if ((long long)g.wK * g.wK * g.n_iso >= (1ll << 32)) return fail(FIC_E_GEOMETRY, "least-squares search: the window has 2^32 candidates or more");
    const size_t P = (size_t)g.planes;
    const int tsz = 64 * g.NR;
    const int tile0 = range_begin / tsz;
    const int tile1 = (range_begin + range_count + tsz - 1) / tsz;
    const int ntiles = tile1 - tile0;
    int nchunks = 1, chunk_len = 0, nslots = 1;
    if (kind == 2) {
        int NR, NC;
        fic_fast_variant(g.B, g.n_iso, &NR, &NC);
        const SweepChunks k = valu_chunks(g.Nd, (long long)ntiles * (g.n_iso / NC) * g.planes, c->opt_chunks, FIC_LSQ_FAST_CHUNK_TARGET, true);
        chunk_len = k.len;
        nchunks = k.nchunks;                           // no empty chunk: every slot gets written
        nslots = fic_lsq_slots(g, nchunks);
    }
    int ct_begin = 0, ct_end = 0, tiles_per_chunk = 0;
    if (kind == 2 && c->opt_lsq_engine == 1) {
        kind = 7;
        c->lsqq.ndtiles = (g.Nd + 31) / 32;
        c->lsqq.nct_alloc = (int)(((long long)g.Nr * g.n_iso + 31) / 32);
        ct_begin = (int)((long long)range_begin * g.n_iso / 32);
        ct_end = (int)(((long long)(range_begin + range_count) * g.n_iso + 31) / 32);
        // fic_lsq_q_chunks.h's fill / balance rule (4 waves per workgroup): no cap on the count, the 22-bit cap on the length
        const LsqQChunks k = lsq_q_chunk_plan(c->lsqq.ndtiles, ct_end - ct_begin, fic_lsq_q_ct(g.B) / 4, g.planes, c->opt_chunks,
                                              FIC_LSQ_Q_NO_CAP, fic_lsq_q_max_tiles_per_chunk(g.B, g.n_iso));
        tiles_per_chunk = k.tiles_per_chunk;
        nslots = nchunks = k.nchunks;
    }
    int rc = c->mem.ensure_zeroed(c->lsq.pool, P * g.Nd_pad * 16, s);      // the tail the prefetch over-reads
    if (rc == FIC_OK) rc = c->mem.ensure(c->lsq.rng, P * g.Nr_pad * 8);
    if (rc == FIC_OK) rc = c->mem.ensure(c->lsq_E, P * g.Nr * 8);
    if (rc) return rc;
    c->lsq.E = c->lsq_E;
    rc = grow_lsq_slots(c, c->lsq.slotE, c->lsq.slotC, (size_t)nslots, P * nslots * g.Nr_pad * 8, P * nslots * g.Nr_pad);
    if (rc) return rc;
    if (fic_launch_scale(c->b.gray, c->b.scaled, g, s)) return fail(FIC_E_HIP, "k_scale launch failed");
    if (fic_launch_pool(c->b.scaled, c->b.pool_pix, c->b.pool_st, c->b.pool_var, c->b.pool_s64, g, s))
        return fail(FIC_E_HIP, "k_pool launch failed");
    rc = c->mem.ensure(c->b.rng_pix, P * g.Nr_pad * g.n_iso * g.DW);
    if (rc) return rc;
    if (fic_launch_range(c->b.gray, c->b.rng_pix, c->b.rng_st, g, s, 1)) return fail(FIC_E_HIP, "k_range launch failed");
    if (fic_launch_lsq_stat(c->b, c->lsq, g, s)) return fail(FIC_E_HIP, "k_lsq_stat launch failed");
    if (kind == 7) {                                   // fragment prep belongs to pool build / range prep: not timed
        const size_t NK = (size_t)g.n / 16;
        rc = c->mem.ensure(c->lsq_q[0], P * c->lsqq.ndtiles * NK * 64 * 16);
        if (rc == FIC_OK) rc = c->mem.ensure(c->lsq_q[1], P * c->lsqq.nct_alloc * NK * 64 * 16);
        if (rc == FIC_OK) rc = c->mem.ensure(c->lsq_q[2], P * g.Nr_pad * sizeof(float));
        if (rc == FIC_OK) rc = c->mem.ensure(c->lsq_q[3], P * g.Nr_pad * sizeof(uint32_t));
        if (rc) return rc;
        c->lsqq.poolQ = c->lsq_q[0], c->lsqq.rngQ = c->lsq_q[1], c->lsqq.rngE = c->lsq_q[2], c->lsqq.rngR = c->lsq_q[3];
        if (fic_launch_lsq_q_prep(c->b, c->lsq, c->lsqq, g, c->opt_lsq_q_eshift, s)) return fail(FIC_E_HIP, "k_lsq_q_prep launch failed");
    }
    rc = c->timer.begin(s);
    if (rc) return rc;
    if (kind == 7) {
        if (fic_launch_sweep_lsq_q(c->b, c->lsq, c->lsqq, g, ct_begin, ct_end, tiles_per_chunk, nchunks, s, c->sweep_stats, c->opt_lsq_widen))
            return fail(FIC_E_HIP, "k_sweep_lsq_q launch failed");
    } else if (kind == 1) {
        if (fic_launch_sweep_lsq_generic(c->b, c->lsq, g, range_begin, range_count, s)) return fail(FIC_E_HIP, "k_sweep_lsq_generic launch failed");
    } else if (fic_launch_sweep_lsq_fast(c->b, c->lsq, g, tile0, ntiles, chunk_len, nchunks, s, c->sweep_stats, c->opt_lsq_widen)) {
        return fail(FIC_E_HIP, "k_sweep_lsq_fast launch failed");
    }
    rc = c->timer.end(s);
    if (rc) return rc;
    if (fic_launch_finalize_lsq(c->b, c->o, c->lsq, nslots, g, range_begin, range_count, s)) return fail(FIC_E_HIP, "k_finalize_lsq launch failed");
    c->last_chunks = nchunks;
    c->last_kind = kind;
    c->last_fused = 0;
    c->last_search = 1;
    c->encoded_any = true;
    return FIC_OK;
}

}  // namespace

extern "C" {

#ifdef FIC_BUILD_XCHECK
const char* fic_version(void) { return "fic-hip 0.5 (gfx950, +xcheck sweeps)"; }
#else
const char* fic_version(void) { return "fic-hip 0.5 (gfx950)"; }
#endif

int fic_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int fic_geometry(int w, int h, int B, int* Rw, int* Rh, int* Dw, int* Dh)
{
    FicGeom g;
    int rc = make_geometry(w, h, B, 1, 1, 1, &g);
    if (rc) return rc;
    if (Rw) *Rw = g.Rw;
    if (Rh) *Rh = g.Rh;
    if (Dw) *Dw = g.Dw;
    if (Dh) *Dh = g.Dh;
    return FIC_OK;
}

int fic_is_greyscale_argb(const int32_t* argb, int w, int h)
{
    if (!argb || w <= 0 || h <= 0) return fail(FIC_E_ARGUMENT, "fic_is_greyscale_argb: bad argument");
    size_t n = (size_t)w * h;
    for (size_t i = 0; i < n; i++) {
        int r = (argb[i] >> 16) & 0xff, g = (argb[i] >> 8) & 0xff, b = argb[i] & 0xff;
        if (r != g || g != b) return 0;
    }
    return 1;
}

fic_ctx* fic_ctx_create(int device, int w, int h, int B, int wK, int n_iso, int planes)
{
    FicGeom g;
    if (make_geometry(w, h, B, wK, n_iso, planes, &g)) return nullptr;
    if (!create_device_ok(device)) return nullptr;
    fic_ctx* c = new fic_ctx();
    c->device = device;
    c->mem.set_device(device);
    c->g = g;
    memset(&c->b, 0, sizeof(c->b));
    memset(&c->o, 0, sizeof(c->o));
    const size_t P = (size_t)planes;
    DevMem& m = c->mem;
    int rc = FIC_OK;
    auto A = [&](int r) { if (rc == FIC_OK) rc = r; };
    A(m.alloc(c->b.scaled, P * g.Ws * g.Hs));
    A(m.alloc(c->b.pool_pix, P * g.Nd_pad * g.n));
    A(m.alloc(c->b.pool_st, P * g.Nd_pad));
    A(m.alloc(c->b.pool_var, P * g.Nd_pad));
    A(m.alloc(c->b.pool_s64, P * g.Nd_pad));
    A(m.alloc(c->b.rng_st, P * g.Nr_pad));
    A(m.alloc(c->b.key, P * g.Nr_pad));
    A(m.alloc(c->o.idx_local, P * g.Nr));
    A(m.alloc(c->o.idx_global, P * g.Nr));
    A(m.alloc(c->o.iso, P * g.Nr));
    A(m.alloc(c->o.a, P * g.Nr));
    A(m.alloc(c->o.b, P * g.Nr));
    A(m.alloc(c->o.err, P * g.Nr));
    A(m.alloc(c->o.qrows, P * g.Nr * 3));
    A(m.alloc(c->o.records, P * g.Nr * 6));
    if (rc == FIC_OK) {
        // zero the pool once: the FIC_POOL_PAD tail blocks stay zero forever (prefetch over-read)
        hipError_t e = hipMemset(c->b.pool_pix, 0, P * g.Nd_pad * g.n);
        if (e == hipSuccess) e = hipMemset(c->b.pool_st, 0, P * g.Nd_pad * sizeof(FicDomStat));
        if (e == hipSuccess) e = hipMemset(c->b.pool_var, 0, P * g.Nd_pad * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMemset(c->b.pool_s64, 0, P * g.Nd_pad * sizeof(double));
        // hipMemset on device memory only ENQUEUES on the null stream; encodes run on the caller's stream, which may be
        // non-blocking (torch's are): without this wait a first encode issued right away can be overtaken by the fill
        // (seen with two processes sharing one GPU: bench.py's post-run check context, round 3)
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        if (e != hipSuccess) rc = fail(FIC_E_HIP, "hipMemset: %s", hipGetErrorString(e));
    }
    if (rc != FIC_OK) {
        delete c;
        return nullptr;
    }
    return c;
}

void fic_ctx_destroy(fic_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    delete c;
}

int fic_ctx_set_gray_host(fic_ctx* c, const uint8_t* gray)
{
    if (!c || !gray) return fail(FIC_E_ARGUMENT, "fic_ctx_set_gray_host: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    if (int rc = upload_input(c, c->gray_own, gray, (size_t)c->g.planes * c->g.W * c->g.H)) return rc;
    c->b.gray = c->gray_own;
    return FIC_OK;
}

int fic_ctx_set_argb_host(fic_ctx* c, const int32_t* argb)
{
    if (!c || !argb) return fail(FIC_E_ARGUMENT, "fic_ctx_set_argb_host: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    if (int rc = upload_argb_as_gray(c, c->argb_stage, c->gray_own, argb, (size_t)c->g.planes * c->g.W * c->g.H)) return rc;
    c->b.gray = c->gray_own;
    return FIC_OK;
}

int fic_ctx_set_gray_device(fic_ctx* c, const void* dev_gray)
{
    if (!c || !dev_gray) return fail(FIC_E_ARGUMENT, "fic_ctx_set_gray_device: null argument");
    // the range preps read the caller's bytes in words of up to 8 bytes (k_prep_q8 / k_range_q8: uint2 rows at B = 8); plane
    // and row offsets keep the base's alignment (W, H multiples of B >= 4; W a multiple of 8 wherever the 8-byte load runs)
    if (int rc = check_input_alignment("fic_ctx_set_gray_device", dev_gray, 8)) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    c->b.gray = (uint8_t*)dev_gray;
    c->have_input = true;
    return FIC_OK;
}

int fic_ctx_encode(fic_ctx* c, int range_begin, int range_count, void* hip_stream)
{
    if (!c) return fail(FIC_E_ARGUMENT, "fic_ctx_encode: null context");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->have_input) return fail(FIC_E_STATE, "fic_ctx_encode: no input image set");
    const FicGeom& g = c->g;
    if (range_count < 0) range_count = g.Nr - range_begin;
    if (range_begin < 0 || range_count < 0 || range_begin + range_count > g.Nr)
        return fail(FIC_E_ARGUMENT, "fic_ctx_encode: range span [%d,%d) outside 0..%d", range_begin, range_begin + range_count, g.Nr);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)hip_stream;
    // another stream than the last encode's: scratch stores, keys and outputs are shared, so the new work starts after the old
    if (int rc = take_stream(c, s)) return rc;
    if (range_count == 0) return FIC_OK;
    if (c->opt_search == 1) return lsq_encode(c, range_begin, range_count, s);

    // which sweep
    int kind = c->opt_sweep;
    if (kind == 0) {
        // Windowed search: the generic kernel.  Full search: the matrix-core sweep k_sweep_q (fic_q.hip) -- same codebook
        // bits as the VALU sweeps, several times faster (north_star's "no MFMA" premise is refuted by
        // the evidence it asked for: profiles/r01z_cfg2_default_pmc_summary.txt, 0.7 % of HBM peak, VALU busy 93.5 %).
        // Very small launches stay on the VALU sweep (no fragment prep).
        // FIC_SWEEP=<n> overrides the automatic choice process-wide wherever kernel n applies ("sweep" option wins);
        // FIC_SWEEP=5 means "the VALU-only default": k_sweep_d4 where it is built, else k_sweep_fast.
        const long long pairs = (long long)g.planes * range_count * g.Nd;
        const int valu = d4_available(g) ? 5 : 2;
        // (k_sweep_q's queue entries carry the domain block in 24 bits: pools of 2^24 blocks or more -- images beyond
        //  16000 x 16000 at B = 8 -- stay on the VALU sweep)
        kind = !g.full ? 1 : ((pairs >= 2000000LL && g.Nd < (1 << 24)) ? 6 : valu);
        const char* env = getenv("FIC_SWEEP");
        if (env && env[0] >= '2' && env[0] <= '6' && env[1] == '\0' && g.full) {
            const int want = env[0] - '0';
            kind = want == 5 ? valu : want;
        }
    }
    if (kind >= 2 && !g.full) return fail(FIC_E_ARGUMENT, "fast sweep needs full search (wK == Dw == Dh)");
#ifndef FIC_BUILD_XCHECK
    if (kind == 3 || kind == 4) return fail(FIC_E_ARGUMENT, "sweep %d (cross-check kernel) is not in this build (FIC_BUILD_XCHECK=0)", kind);
#endif
    if (kind == 5 && !d4_available(g)) return fail(FIC_E_ARGUMENT, "sweep 5 (k_sweep_d4) needs full search, n_iso = 8 and B = 8");
    if (kind == 6 && g.Nd >= (1 << 24)) return fail(FIC_E_ARGUMENT, "sweep 6 (k_sweep_q) needs a pool of fewer than 2^24 blocks");
    const int tsz = 64 * g.NR;
    const int tile0 = range_begin / tsz;
    const int tile1 = (range_begin + range_count + tsz - 1) / tsz;
    const int ntiles = tile1 - tile0;
    int nchunks = 1;
    int rc = FIC_OK;
    // pool build (createCodebuch FC:119) + range prep
    // (a small launch of the default sweep builds the scaled image inside its one fused prep kernel: fic_q.hip, k_prep_q8)
    bool fused_prep = false;
    if (kind == 6) {
        const QShape q = q_shape(g);
        fused_prep = fic_q_prep_fused(g, q.ndtiles_alloc, tile1 * (64 * g.NR) / 64 - tile0 * (64 * g.NR) / 64) != 0;
    }
    if (!fused_prep && fic_launch_scale(c->b.gray, c->b.scaled, g, s)) return fail(FIC_E_HIP, "k_scale launch failed");
    if (kind == 6) {
        // fused: k_pool_q = pool + statistics + A fragments, k_range_q = range statistics + key reset + copies + B fragments
        rc = q_prep(c, tile0, tile1, s);
    } else {
        if (fic_launch_pool(c->b.scaled, c->b.pool_pix, c->b.pool_st, c->b.pool_var, c->b.pool_s64, g, s))
            return fail(FIC_E_HIP, "k_pool launch failed");
        // the lane-transposed store of range blocks + isometry copies: only these sweeps read it (134 MB at 4096x4096 with
        // 8 isometries), so it is allocated on their first use, not with the context
        if (kind != 5) {
            const int rca = c->mem.ensure(c->b.rng_pix, (size_t)g.planes * g.Nr_pad * g.n_iso * g.DW);
            if (rca) return rca;
        }
        // k_sweep_d4 reads its own slot store and the finaliser reads the image: no isometry copies to build then
        if (fic_launch_range(c->b.gray, c->b.rng_pix, c->b.rng_st, g, s, kind == 5 ? 0 : 1)) return fail(FIC_E_HIP, "k_range launch failed");
        // one 2-D fill: rows = planes (pitch Nr_pad keys), width = the tile span of this shard
        HIP_TRY(hipMemset2DAsync(c->b.key + (size_t)tile0 * tsz, (size_t)g.Nr_pad * sizeof(unsigned long long), 0xFF,
                                 (size_t)ntiles * tsz * sizeof(unsigned long long), (size_t)g.planes, s));
        if (kind == 5) rc = d4_prep(c, s);
        else if (kind >= 3) rc = matrix_core_prep(c, kind, s);          // fragment prep belongs to pool build / range prep: not timed
    }
    if (rc == FIC_OK) rc = c->timer.begin(s);
    if (rc == FIC_OK) {
        if (kind == 1) {
            if (fic_launch_sweep_generic(c->b, g, range_begin, range_count, s)) rc = fail(FIC_E_HIP, "k_sweep_generic launch failed");
        } else if (kind == 6) {
            rc = q_sweep(c, tile0, tile1, s, &nchunks, fused_prep, range_begin, range_count);   // small launches: finalise in the sweep's tail
        } else if (kind == 5) {
            rc = d4_sweep(c, tile0, tile1 - tile0, s, &nchunks);
        } else if (kind >= 3) {
            rc = matrix_core_sweep(c, kind, tile0, tile1, s, &nchunks);
        } else {
            rc = valu_sweep(c, tile0, tile1 - tile0, s, &nchunks);
        }
    }
    if (rc == FIC_OK) rc = c->timer.end(s);
    if (rc != FIC_OK) return rc;
    c->last_chunks = nchunks;
    c->last_kind = kind;
    c->last_fused = fused_prep ? 1 : 0;
    c->last_search = 0;
    // kinds 5 and 6 build no lane-transposed isometry copies: the finaliser recomputes the winner's covariance from the image
    if (!fused_prep &&
        fic_launch_finalize(c->b, c->o, g, range_begin, range_count, s, (kind == 5 || kind == 6) ? 1 : 0)) return fail(FIC_E_HIP, "k_finalize launch failed");
    c->encoded_any = true;
    return FIC_OK;
}

int fic_ctx_sync(fic_ctx* c)
{
    if (!c) return fail(FIC_E_ARGUMENT, "fic_ctx_sync: null context");
    return ctx_sync(c);
}

int fic_ctx_get_results_host(fic_ctx* c, int32_t* idx_local, float* a, float* b, int32_t* iso, int32_t* qrows,
                             int32_t* idx_global, float* err)
{
    if (!c) return fail(FIC_E_ARGUMENT, "fic_ctx_get_results_host: null context");
    if (!c->encoded_any) return fail(FIC_E_STATE, "fic_ctx_get_results_host: nothing encoded yet");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->last_stream));
    size_t n = (size_t)c->g.planes * c->g.Nr;
    // idx_local / a / b / iso / qrows are the six words of the packed 24-byte record (finalize_store): ONE copy into a pinned
    // buffer of the context and an unpack on the host instead of up to five blocking copies of ~15 us each -- the one-shot entry
    // the JNI host calls (fic_encode_gray_*) is three of them shorter per call.
    // (up to 65 536 range blocks: beyond that the copies' latency no longer matters and the host loop would)
    if (n > (size_t)65536) {
        if (idx_local) HIP_TRY(hipMemcpy(idx_local, c->o.idx_local, n * 4, hipMemcpyDeviceToHost));
        if (a) HIP_TRY(hipMemcpy(a, c->o.a, n * 4, hipMemcpyDeviceToHost));
        if (b) HIP_TRY(hipMemcpy(b, c->o.b, n * 4, hipMemcpyDeviceToHost));
        if (iso) HIP_TRY(hipMemcpy(iso, c->o.iso, n * 4, hipMemcpyDeviceToHost));
        if (qrows) HIP_TRY(hipMemcpy(qrows, c->o.qrows, n * 12, hipMemcpyDeviceToHost));
    } else if (idx_local || a || b || iso || qrows) {
        std::lock_guard<std::mutex> lk(c->mu);
        if (int rc = c->mem.ensure(c->host_rec, n * 6, kMemPinned)) return rc;
        HIP_TRY(hipMemcpy(c->host_rec, c->o.records, n * 6 * sizeof(int32_t), hipMemcpyDeviceToHost));
        const int32_t* r = c->host_rec;
        for (size_t i = 0; i < n; i++, r += 6) {
            if (idx_local) idx_local[i] = r[0];
            if (a) memcpy(&a[i], &r[1], 4);
            if (b) memcpy(&b[i], &r[2], 4);
            if (iso) iso[i] = r[3];
            if (qrows) { qrows[3 * i] = r[0]; qrows[3 * i + 1] = r[4]; qrows[3 * i + 2] = r[5]; }
        }
    }
    if (idx_global) HIP_TRY(hipMemcpy(idx_global, c->o.idx_global, n * 4, hipMemcpyDeviceToHost));
    if (err) HIP_TRY(hipMemcpy(err, c->o.err, n * 4, hipMemcpyDeviceToHost));
    return FIC_OK;
}

int fic_ctx_result_device_ptrs(fic_ctx* c, void** idx_local, void** a, void** b, void** iso, void** qrows,
                               void** idx_global, void** err)
{
    if (!c) return fail(FIC_E_ARGUMENT, "fic_ctx_result_device_ptrs: null context");
    if (idx_local) *idx_local = c->o.idx_local;
    if (a) *a = c->o.a;
    if (b) *b = c->o.b;
    if (iso) *iso = c->o.iso;
    if (qrows) *qrows = c->o.qrows;
    if (idx_global) *idx_global = c->o.idx_global;
    if (err) *err = c->o.err;
    return FIC_OK;
}

int fic_ctx_records_device_ptr(fic_ctx* c, void** records)
{
    if (!c || !records) return fail(FIC_E_ARGUMENT, "fic_ctx_records_device_ptr: null argument");
    *records = c->o.records;
    return FIC_OK;
}

int fic_ctx_collage_host(fic_ctx* c, int32_t* argb_out)
{
    if (!c || !argb_out) return fail(FIC_E_ARGUMENT, "fic_ctx_collage_host: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->encoded_any) return fail(FIC_E_STATE, "fic_ctx_collage_host: nothing encoded yet");
    HIP_TRY(hipSetDevice(c->device));
    size_t npix = (size_t)c->g.planes * c->g.W * c->g.H;
    if (int rc = c->mem.ensure(c->collage, npix)) return rc;
    if (fic_launch_collage(c->b, c->o, c->collage, c->g, c->last_stream)) return fail(FIC_E_HIP, "k_collage launch failed");
    HIP_TRY(hipStreamSynchronize(c->last_stream));
    HIP_TRY(hipMemcpy(argb_out, c->collage, npix * sizeof(int32_t), hipMemcpyDeviceToHost));
    return FIC_OK;
}

int fic_ctx_set_option(fic_ctx* c, const char* name, int value)
{
    if (!c || !name) return fail(FIC_E_ARGUMENT, "fic_ctx_set_option: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    // this handle's own options; every other name is the core's (fic_ctx_options.h)
    if (!strcmp(name, "sweep")) {
        if (c->opt_search == 1 && (value < 0 || value > 2))
            return fail(FIC_E_ARGUMENT, "sweep must be 0 (auto), 1 (generic) or 2 (fast) under the least-squares search (\"search\" = 1)");
        if (value < 0 || value > 6)
            return fail(FIC_E_ARGUMENT, "sweep must be 0 (auto), 1 (generic), 2 (fast, VALU), 3 (matrix-core, exact covariances), 4 (matrix-core, i8 operands), 5 (VALU, group-Fourier isometries) or 6 (matrix-core, normalised f16 prune GEMM)");
        c->opt_sweep = value;
        return FIC_OK;
    }
    if (!strcmp(name, "q_shape")) {                    // MFMA shape of the 1-isometry k_sweep_q at B = 8 / 16 (tests, A/B runs)
        if (value < 0 || value > 2) return fail(FIC_E_ARGUMENT, "q_shape must be 0 (by pool size), 1 (16x16x32) or 2 (32x32x16)");
        c->g.q_shape = value;
        return FIC_OK;
    }
    if (!strcmp(name, "q_noflag")) {                   // diagnostic: k_sweep_q without any flagged tile (wrong codebooks): its floor
        c->opt_noflag = value ? 1 : 0;
        return FIC_OK;
    }
    if (!strcmp(name, "search") && value == 1 && c->opt_sweep > 2)
        return fail(FIC_E_ARGUMENT, "the least-squares search (\"search\" = 1) has sweeps 0 (auto), 1 (generic) and 2 (fast), not %d", c->opt_sweep);
    return set_core_option(c, kOptGrey, "", name, value);
}

int fic_ctx_sweep_time(fic_ctx* c, double* total_ms, int* launches, int reset)
{
    if (!c) return fail(FIC_E_ARGUMENT, "fic_ctx_sweep_time: null context");
    return ctx_sweep_time(c, total_ms, launches, reset);
}

int fic_ctx_sweep_stats(fic_ctx* c, uint64_t* out8, int reset)
{
    if (!c || !out8) return fail(FIC_E_ARGUMENT, "fic_ctx_sweep_stats: null argument");
    return ctx_sweep_stats(c, "fic_ctx_sweep_stats", out8, reset);
}

int fic_ctx_info(fic_ctx* c, int* out10)
{
    if (!c || !out10) return fail(FIC_E_ARGUMENT, "fic_ctx_info: null argument");
    const FicGeom& g = c->g;
    int v[10] = {g.Rw, g.Rh, g.Nr, g.Dw, g.Dh, g.Nd, g.NR, g.tiles, c->last_chunks, c->last_kind};
    memcpy(out10, v, sizeof(v));
    return FIC_OK;
}

int fic_ctx_last_kernel(fic_ctx* c, char* out, int capacity)
{
    if (!c || !out || capacity < 1) return fail(FIC_E_ARGUMENT, "fic_ctx_last_kernel: bad argument");
    const FicGeom& g = c->g;
    const int NK = g.n / 16, kind = c->last_kind;
    const char* multi = c->last_chunks > 1 ? "true" : "false";
    const bool shorts = kind == 6 && fic_q_multi_kind(c->last_chunks, c->last_tiles_per_chunk) == 2;    // short pool chunks: k_sweep_qs / k_sweep_q16s
    char buf[96];
    if (kind == 6 && fic_q_shape16(g) && shorts) snprintf(buf, sizeof(buf), "k_sweep_q16s<%d>", NK);
    else if (kind == 6 && fic_q_shape16(g)) snprintf(buf, sizeof(buf), "k_sweep_q16<%d, %s>", NK, multi);
    else if (kind == 6 && shorts) snprintf(buf, sizeof(buf), "k_sweep_qs<%d, %d>", NK, g.n_iso == 1 ? 0 : (g.B == 4 ? 1 : 2));
    else if (kind == 6) snprintf(buf, sizeof(buf), "k_sweep_q<%d, %d, %s>", NK, g.n_iso == 1 ? 0 : (g.B == 4 ? 1 : 2), multi);
    else if (c->last_search == 1 && kind == 7) snprintf(buf, sizeof(buf), "k_sweep_lsq_q<%d, %d>", NK, g.n_iso == 8 ? 3 : 0);
    else if (c->last_search == 1) snprintf(buf, sizeof(buf), kind == 2 ? "k_sweep_lsq_fast" : "k_sweep_lsq_generic");
    else if (kind == 5) snprintf(buf, sizeof(buf), "k_sweep_d4");
    else if (kind == 2) snprintf(buf, sizeof(buf), "k_sweep_fast");
    else if (kind == 1) snprintf(buf, sizeof(buf), "k_sweep_generic");
    else if (kind == 3 || kind == 4) {
        const bool bf16 = kind == 3 && (g.B <= 8 || g.n_iso == 8);
        snprintf(buf, sizeof(buf), "%s%s", bf16 ? "k_sweep_bf16" : "k_sweep_mfma", g.n_iso == 8 ? "" : (bf16 ? "_1" : "1"));
    } else snprintf(buf, sizeof(buf), "(none)");
    // a small launch of the default sweep: one fused prep kernel before it, k_finalize's work in its tail (2 kernels, not 5)
    snprintf(out, (size_t)capacity, "%s%s", buf, kind == 6 && c->last_fused ? " after k_prep_q8, finalising" : "");
    return FIC_OK;
}

int fic_sweep_ranges_per_pool_read(int kind, int B, int n_iso)
{
    if ((B != 4 && B != 8 && B != 16) || (n_iso != 1 && n_iso != 8)) return 0;
    if (kind == 6) return fic_q_ctw_host(B) * 32 / fic_q_cols_per_range(B, n_iso);
    if (kind == 2 || kind == 5) {
        int NR = 1, NC = 1;
        fic_fast_variant(B, n_iso, &NR, &NC);
        return 64 * (kind == 5 ? 1 : NR);
    }
    return 0;
}

int fic_debug_sqrt_f64(int device, uint32_t first, uint32_t count, double* out)
{
    if (!out || count == 0) return fail(FIC_E_ARGUMENT, "fic_debug_sqrt_f64: bad argument");
    int rc = check_device(device);
    if (rc) return rc;
    DevMem scratch(device);
    double* d = nullptr;
    rc = scratch.alloc(d, count);
    if (rc) return rc;
    if (fic_launch_sqrt_probe(d, first, count, nullptr)) return fail(FIC_E_HIP, "k_sqrt_probe launch failed");
    const hipError_t e = hipMemcpy(out, d, (size_t)count * sizeof(double), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(FIC_E_HIP, "hipMemcpy: %s", hipGetErrorString(e));
    return FIC_OK;
}

int fic_ctx_debug_pool_host(fic_ctx* c, uint8_t* pix, uint32_t* sum, uint32_t* var, uint8_t* scaled)
{
    if (!c) return fail(FIC_E_ARGUMENT, "fic_ctx_debug_pool_host: null context");
    if (!c->encoded_any) return fail(FIC_E_STATE, "fic_ctx_debug_pool_host: nothing encoded yet");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->last_stream));
    const FicGeom& g = c->g;
    for (int p = 0; p < g.planes; p++) {
        if (pix)
            HIP_TRY(hipMemcpy(pix + (size_t)p * g.Nd * g.n, c->b.pool_pix + (size_t)p * g.Nd_pad * g.n, (size_t)g.Nd * g.n,
                              hipMemcpyDeviceToHost));
        if (var)
            HIP_TRY(hipMemcpy(var + (size_t)p * g.Nd, c->b.pool_var + (size_t)p * g.Nd_pad, (size_t)g.Nd * 4,
                              hipMemcpyDeviceToHost));
        if (sum) {
            std::vector<FicDomStat> st(g.Nd);
            HIP_TRY(hipMemcpy(st.data(), c->b.pool_st + (size_t)p * g.Nd_pad, (size_t)g.Nd * sizeof(FicDomStat),
                              hipMemcpyDeviceToHost));
            for (int i = 0; i < g.Nd; i++) sum[(size_t)p * g.Nd + i] = st[i].sum;
        }
    }
    if (scaled) HIP_TRY(hipMemcpy(scaled, c->b.scaled, (size_t)g.planes * g.Ws * g.Hs, hipMemcpyDeviceToHost));
    return FIC_OK;
}

int fic_ctx_debug_q_host(fic_ctx* c, int which, void* out, int64_t capacity, int64_t* size)
{
    if (!c || !size) return fail(FIC_E_ARGUMENT, "fic_ctx_debug_q_host: null argument");
    if (!c->encoded_any || !c->q_pool) return fail(FIC_E_STATE, "fic_ctx_debug_q_host: no encode through the default sweep (\"sweep\" = 6) yet");
    const void* const stores[6] = {c->q_pool, c->q_flat, c->q_rng, c->q_E, c->b.rng_st, c->q_rngC};
    return debug_store_host(c, "fic_ctx_debug_q_host", stores, 6, which, out, capacity, size);
}

int fic_ctx_debug_lsq_q_host(fic_ctx* c, int which, void* out, int64_t capacity, int64_t* size)
{
    if (!c || !size) return fail(FIC_E_ARGUMENT, "fic_ctx_debug_lsq_q_host: null argument");
    return ctx_debug_lsq_q(c, "fic_ctx_debug_lsq_q_host", which, out, capacity, size);
}

}  // extern "C"

int ficd::encode_oneshot(const uint8_t* gray, const int32_t* argb, int w, int h, int B, int wK, int n_iso, int device,
                          int32_t* idx_local, float* a, float* b, int32_t* iso, int32_t* qrows, int64_t* E, int search)
{
    if ((!gray && !argb) || !idx_local || !a || !b) return fail(FIC_E_ARGUMENT, "%s: null argument", search ? "fic_encode_gray_lsq" : "fic_encode_gray");
    // The GUI calls encode once per slider move with the same geometry (CTL:125-145): keep the last few
    // working sets instead of paying ~18 device allocations and frees per call.
    Lease<fic_ctx> L;
    int rc = L.open(device, w, h, B, wK, n_iso, search);
    if (rc == FIC_OK) rc = gray ? fic_ctx_set_gray_host(L.c, gray) : fic_ctx_set_argb_host(L.c, argb);
    if (rc == FIC_OK) rc = fic_ctx_encode(L.c, 0, -1, nullptr);
    if (rc == FIC_OK) rc = fic_ctx_get_results_host(L.c, idx_local, a, b, iso, qrows, nullptr, nullptr);
    if (rc == FIC_OK && E) rc = fic_ctx_get_lsq_error_host(L.c, E);
    return L.close(rc);
}

extern "C" {

void fic_release_cache(void)
{
    g_idle_grey.drain();
    g_idle_rgb.drain();
    release_comms();
    release_decoder_arenas();
}

int fic_encode_gray_argb(const int32_t* argb, int w, int h, int B, int wK, int n_iso, int device, int32_t* idx_local,
                         float* a, float* b, int32_t* iso, int32_t* qrows)
{
    return encode_oneshot(nullptr, argb, w, h, B, wK, n_iso, device, idx_local, a, b, iso, qrows);
}

int fic_encode_gray_u8(const uint8_t* gray, int w, int h, int B, int wK, int n_iso, int device, int32_t* idx_local,
                       float* a, float* b, int32_t* iso, int32_t* qrows)
{
    return encode_oneshot(gray, nullptr, w, h, B, wK, n_iso, device, idx_local, a, b, iso, qrows);
}

}  // extern "C"
