// fic_capi_rgb_lsq.cpp -- C ABI of the least-squares domain search of the joint-RGB path: the encode
// of a colour context under "search" = 1 (kernels in fic_lsq_rgb.hip) and the winners' errors.  The one-shot entry is
// fic_capi_rgb.cpp's on a lease under "search" = 1; the quadtree entries are in fic_capi_quadtree.cpp.  Host-side orchestration only.
#include "fic_internal.h"
#include "fic_lsq_q_chunks.h"
#include "fic_sweep_chunks.h"

using namespace ficd;

// scaleImageRGB as for the reference's search, then the planar byte stores and sums, k_sweep_lsq_rgb_generic (windows, B = 16,
// "sweep" = 1) or k_sweep_lsq_rgb_fast (full search at B <= 8), k_finalize_lsq_rgb and the reference's collage of the rows.
// Under "lsq_engine" = 1 a full search with "sweep" 0 or 2 at B = 4 / 8 / 16 runs k_sweep_lsq_rgb_q instead:
// where the fast sweep would run at B <= 8, and where the automatic choice would take the generic kernel at B = 16 ("sweep" = 2
// is accepted there only under this option).  "sweep" = 1, windows and "search" = 0 never see the option.
int ficd::rgb_lsq_encode(fic_rgb_ctx* c, int with_collage, hipStream_t s)
{
    const FicGeom& g = c->g;
    int NC = 1;
    const bool fast_ok = g.full && fic_lsq_rgb_variant(g.B, g.n_iso, &NC) == 0;
    int kind = c->opt_sweep;
    const bool q_ok = c->opt_lsq_engine == 1 && g.full && kind != 1 && (g.B == 4 || g.B == 8 || g.B == 16) && (g.n_iso == 1 || g.n_iso == 8);
    if (q_ok) kind = 7;
    if (kind == 0) kind = fast_ok ? 2 : 1;
    if (kind == 2 && !fast_ok)
        return fail(FIC_E_ARGUMENT, "least-squares search: the fast sweep (\"sweep\" = 2) needs full search (wK == Dw == Dh) and B <= 8");
    const size_t P = (size_t)g.planes;
    FicLsqRgb& q = c->lsq;
    q.Nr_pad = (g.Nr + 63) / 64 * 64;
    const size_t nrp = (size_t)q.Nr_pad;
    int nchunks = 1, chunk_len = g.Nd, nslots = 1;
    if (kind == 2) {
        const SweepChunks k = rgb_lsq_fast_chunks(g.Nd, (long long)(q.Nr_pad / 64) * (g.n_iso / NC) * g.planes, c->opt_chunks);
        chunk_len = k.len;
        nchunks = k.nchunks;                           // no empty chunk: every slot gets written
        nslots = fic_lsq_rgb_slots(g, nchunks);
    }
    LsqRgbQPlan plan{};
    if (kind == 7) {
        plan = lsq_rgb_q_plan(g.Nd, (long long)g.Nr * g.n_iso, g.B, g.n_iso, g.planes, c->opt_chunks);
        if (!plan.ok) return fail(FIC_E_GEOMETRY, "least-squares search on the matrix cores: the pool has 2^32 - 1 candidates or more");
        nchunks = plan.nchunks;
        nslots = plan.nslots;
        c->lsqq.ndtiles = plan.ndtiles;
        c->lsqq.nct = (int)(((long long)g.Nr * g.n_iso + 31) / 32);
    }
    DevMem& m = c->mem;
    int rc = m.ensure_zeroed(q.pool3, P * g.Nd_pad * 3 * g.n, s);
    if (rc == FIC_OK) rc = m.ensure_zeroed(q.pool_st, P * g.Nd_pad * 32, s);
    if (rc == FIC_OK) rc = m.ensure_zeroed(q.rng3, P * nrp * g.n_iso * 3 * g.n, s);      // the lanes past N_r of the last tile read zeros
    if (rc == FIC_OK) rc = m.ensure_zeroed(q.rng_st, P * nrp * 16, s);
    if (rc == FIC_OK) rc = m.ensure(c->lsq_E, P * g.Nr * 8);
    if (rc) return rc;
    q.E = c->lsq_E;
    rc = grow_lsq_slots(c, q.slotE, q.slotC, (size_t)nslots, P * nslots * nrp * 8, P * nslots * nrp);
    if (rc) return rc;
    FicRgbOutputs o;                                   // image 0 of the batch: the kernels take the image from their grid
    o.idx_local = c->idx_local; o.idx_global = c->idx_global; o.a = c->a; o.bR = c->bR; o.bG = c->bG; o.bB = c->bB;
    o.qrows = c->qrows; o.iso = c->iso;
    if (fic_launch_scale_rgb_planes(c->argb, c->scaled, g, s)) return fail(FIC_E_HIP, "k_scale_rgb launch failed");
    if (fic_launch_lsq_rgb_prep(c->argb, c->scaled, q, g, s)) return fail(FIC_E_HIP, "k_lsq_rgb_prep launch failed");
    if (kind == 7) {                                   // fragment prep belongs to the stores: not timed
        const size_t NK = 3 * (size_t)g.n / 16;
        FicLsqRgbQ& f = c->lsqq;
        rc = m.ensure(c->lsq_q[0], P * f.ndtiles * NK * 64 * 16);
        if (rc == FIC_OK) rc = m.ensure(c->lsq_q[1], P * f.nct * NK * 64 * 16);
        if (rc == FIC_OK) rc = m.ensure(c->lsq_q[2], P * nrp * sizeof(float));
        if (rc == FIC_OK) rc = m.ensure(c->lsq_q[3], P * nrp * sizeof(uint32_t));
        if (rc) return rc;
        f.poolQ = c->lsq_q[0], f.rngQ = c->lsq_q[1], f.rngE = c->lsq_q[2], f.rngR = c->lsq_q[3];
        if (fic_launch_lsq_rgb_q_prep(q, f, g, c->opt_lsq_q_eshift, s)) return fail(FIC_E_HIP, "k_lsq_rgb_q_prep launch failed");
    }
    rc = c->timer.begin(s);
    if (rc) return rc;
    if (kind == 7) {
        if (fic_launch_sweep_lsq_rgb_q(q, c->lsqq, g, plan.tiles_per_chunk, plan.nchunks, s, c->sweep_stats, c->opt_lsq_widen))
            return fail(FIC_E_HIP, "k_sweep_lsq_rgb_q launch failed");
    } else if (kind == 1) {
        if (fic_launch_sweep_lsq_rgb_generic(q, g, s)) return fail(FIC_E_HIP, "k_sweep_lsq_rgb_generic launch failed");
    } else if (fic_launch_sweep_lsq_rgb_fast(q, g, chunk_len, nchunks, s, c->sweep_stats, c->opt_lsq_widen)) {
        return fail(FIC_E_HIP, "k_sweep_lsq_rgb_fast launch failed");
    }
    rc = c->timer.end(s);
    if (rc) return rc;
    if (fic_launch_finalize_lsq_rgb(o, q, nslots, g, s)) return fail(FIC_E_HIP, "k_finalize_lsq_rgb launch failed");
    if (with_collage && fic_launch_rgb_collage(c->scaled, o, c->collage, g, s)) return fail(FIC_E_HIP, "k_collage_rgb launch failed");
    c->last_sweep = 1;                                 // nothing of the matrix-core sweep to look at (fic_rgb_ctx_debug_q_host)
    c->last_search = 1;
    c->last_lsq_kind = kind;
    c->last_lsq_chunks = nchunks;
    c->encoded_any = true;
    c->have_collage = with_collage != 0;
    return FIC_OK;
}

extern "C" {

int fic_rgb_ctx_get_lsq_error_host(fic_rgb_ctx* c, int64_t* E)
{
    if (!c || !E) return fail(FIC_E_ARGUMENT, "fic_rgb_ctx_get_lsq_error_host: null argument");
    return ctx_get_lsq_error(c, "fic_rgb_ctx_get_lsq_error_host", E);
}

int fic_rgb_ctx_sweep_time(fic_rgb_ctx* c, double* total_ms, int* launches, int reset)
{
    if (!c) return fail(FIC_E_ARGUMENT, "fic_rgb_ctx_sweep_time: null context");
    return ctx_sweep_time(c, total_ms, launches, reset);
}

int fic_rgb_ctx_last_lsq_chunks(fic_rgb_ctx* c)
{
    if (!c) return fail(FIC_E_ARGUMENT, "fic_rgb_ctx_last_lsq_chunks: null context");
    return c->last_search == 1 ? c->last_lsq_chunks : 0;
}

int fic_rgb_ctx_debug_lsq_q_host(fic_rgb_ctx* c, int which, void* out, int64_t capacity, int64_t* size)
{
    if (!c || !size) return fail(FIC_E_ARGUMENT, "fic_rgb_ctx_debug_lsq_q_host: null argument");
    return ctx_debug_lsq_q(c, "fic_rgb_ctx_debug_lsq_q_host", which, out, capacity, size);
}

}  // extern "C"
