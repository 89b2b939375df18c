// fic_capi_rgb_lsq.cpp -- C ABI of the least-squares domain search of the joint-RGB path: the encode
// of a colour context under "search" = 1 (kernels in fic_lsq_rgb.hip), the winners' errors and the one-shot entry over the
// cached contexts.  The quadtree entries are in fic_capi_quadtree.cpp.  Host-side orchestration only.
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
    if (rc == FIC_OK) rc = m.ensure(q.E, P * g.Nr * 8);
    if (rc) return rc;
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
        rc = m.ensure(f.poolQ, P * f.ndtiles * NK * 64 * 16);
        if (rc == FIC_OK) rc = m.ensure(f.rngQ, P * f.nct * NK * 64 * 16);
        if (rc == FIC_OK) rc = m.ensure(f.rngE, P * nrp * sizeof(float));
        if (rc == FIC_OK) rc = m.ensure(f.rngR, P * nrp * sizeof(uint32_t));
        if (rc) return rc;
        if (fic_launch_lsq_rgb_q_prep(q, f, g, c->opt_lsq_q_eshift, s)) return fail(FIC_E_HIP, "k_lsq_rgb_q_prep launch failed");
    }
    rc = c->timer.begin(s);
    if (rc) return rc;
    if (kind == 7) {
        if (fic_launch_sweep_lsq_rgb_q(q, c->lsqq, g, plan.tiles_per_chunk, plan.nchunks, s, c->q.stats, c->opt_lsq_widen))
            return fail(FIC_E_HIP, "k_sweep_lsq_rgb_q launch failed");
    } else if (kind == 1) {
        if (fic_launch_sweep_lsq_rgb_generic(q, g, s)) return fail(FIC_E_HIP, "k_sweep_lsq_rgb_generic launch failed");
    } else if (fic_launch_sweep_lsq_rgb_fast(q, g, chunk_len, nchunks, s, c->q.stats, c->opt_lsq_widen)) {
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
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->encoded_any || c->last_search != 1 || !c->lsq.E)
        return fail(FIC_E_STATE, "fic_rgb_ctx_get_lsq_error_host: the last encode was not a least-squares search (\"search\" = 1)");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->last_stream));
    static_assert(sizeof(long long) == sizeof(int64_t), "E");
    HIP_TRY(hipMemcpy(E, c->lsq.E, (size_t)c->g.planes * c->g.Nr * sizeof(int64_t), hipMemcpyDeviceToHost));
    return FIC_OK;
}

int fic_rgb_ctx_sweep_time(fic_rgb_ctx* c, double* total_ms, int* launches, int reset)
{
    if (!c) return fail(FIC_E_ARGUMENT, "fic_rgb_ctx_sweep_time: null context");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    return c->timer.read(total_ms, launches, reset);
}

int fic_rgb_ctx_last_lsq_chunks(fic_rgb_ctx* c)
{
    if (!c) return fail(FIC_E_ARGUMENT, "fic_rgb_ctx_last_lsq_chunks: null context");
    return c->last_search == 1 ? c->last_lsq_chunks : 0;
}

int fic_rgb_ctx_debug_lsq_q_host(fic_rgb_ctx* c, int which, void* out, int64_t capacity, int64_t* size)
{
    if (!c || !size) return fail(FIC_E_ARGUMENT, "fic_rgb_ctx_debug_lsq_q_host: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->encoded_any || !c->lsqq.poolQ)
        return fail(FIC_E_STATE, "fic_rgb_ctx_debug_lsq_q_host: no encode through the matrix-core least-squares sweep (\"lsq_engine\" = 1) yet");
    const void* const stores[4] = {c->lsqq.poolQ, c->lsqq.rngQ, c->lsqq.rngE, c->lsqq.rngR};
    return debug_store_host(c, "fic_rgb_ctx_debug_lsq_q_host", stores, 4, which, out, capacity, size);
}

int fic_encode_rgb_lsq_argb(const int32_t* argb, int w, int h, int B, int wK, int n_iso, int device, int32_t* idx_local, float* a,
                            float* bR, float* bG, float* bB, int32_t* iso, int32_t* qrows5, int32_t* collage_argb, int64_t* E)
{
    if (!argb || !idx_local || !a || !bR || !bG || !bB) return fail(FIC_E_ARGUMENT, "fic_encode_rgb_lsq_argb: null argument");
    if (n_iso != 1 && n_iso != 8) return fail(FIC_E_ARGUMENT, "n_iso=%d: the joint-RGB path has 1 or 8 isometries", n_iso);
    fic_rgb_ctx* c = g_idle_rgb.take(device, w, h, B, wK, n_iso);
    if (!c) c = fic_rgb_ctx_create_iso(device, w, h, B, wK, n_iso, 1);
    if (!c) return g_err_code ? g_err_code : FIC_E_HIP;   // fic_rgb_ctx_create_iso recorded why
    int rc = fic_rgb_ctx_set_option(c, "search", 1);
    if (rc == FIC_OK) rc = fic_rgb_ctx_set_argb_host(c, argb);
    if (rc == FIC_OK) rc = fic_rgb_ctx_encode(c, collage_argb ? 1 : 0, nullptr);
    if (rc == FIC_OK) rc = fic_rgb_ctx_get_results_host(c, idx_local, a, bR, bG, bB, qrows5, collage_argb);
    if (rc == FIC_OK && iso) rc = fic_rgb_ctx_get_iso_host(c, iso);
    if (rc == FIC_OK && E) rc = fic_rgb_ctx_get_lsq_error_host(c, E);
    ErrKeep keep;
    // the cached contexts serve the reference entries too: never parked in least-squares mode
    if (rc == FIC_OK && fic_rgb_ctx_set_option(c, "search", 0) == FIC_OK) g_idle_rgb.give(c);
    else fic_rgb_ctx_destroy(c);
    return rc;
}

}  // extern "C"
