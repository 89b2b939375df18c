// fic_capi_rgb.cpp -- C ABI, joint-RGB path: encodeRGB (FC:171-219) as one-shot entry and as batched device-resident
// contexts (fic_rgb_ctx_*), decodeRGB from a context's codebook (on the decode job of fic_capi_decode.cpp).  Host-side orchestration only.
#include "fic_internal.h"
#include "fic_sweep_chunks.h"

using namespace ficd;

IdleCache<fic_rgb_ctx, 4> ficd::g_idle_rgb;

extern "C" {

// ---- joint-RGB encode (encodeRGB FC:171-219) -----------------------------------------------------
// A context (fic_rgb_ctx, fic_internal.h) owns the device working set of `planes` colour images of one geometry (config-5 style
// batches; the one-shot entry keeps a few single-image contexts).  The covariance sums stay sequential f32 in the reference's
// order (FC:781-792: they exceed 2^24).
namespace {
// buffers of plane p as the per-image kernels expect them
void rgb_plane(const fic_rgb_ctx* c, int p, FicRgbBuffers* b, FicRgbOutputs* o)
{
    const FicGeom& g = c->g;
    const size_t P = (size_t)p, nd = (size_t)g.Nd, nr = (size_t)g.Nr, n = (size_t)g.n;
    b->argb = const_cast<int32_t*>(c->argb) + P * g.W * g.H;
    b->scaled = c->scaled + P * g.Ws * g.Hs;
    b->pool_sum = c->pool_sum + P * nd * n;
    b->pool_cf = c->pool_cf ? c->pool_cf + P * nd * n : nullptr;
    b->pool_st = c->pool_st + P * nd;
    b->rng_t = c->rng_t + P * nr * n;
    b->rng_st = c->rng_st + P * nr;
    b->key = c->key + P * nr;
    o->idx_local = c->idx_local + P * nr;
    o->idx_global = c->idx_global + P * nr;
    o->a = c->a + P * nr;
    o->bR = c->bR + P * nr;
    o->bG = c->bG + P * nr;
    o->bB = c->bB + P * nr;
    o->qrows = c->qrows + P * nr * 5;
    o->iso = c->iso ? c->iso + P * nr : nullptr;
}
// pool chunks of the matrix-core full search: fic_sweep_chunks.h's rule of k_sweep_q (one image at a time), or the "chunks" option
void rgb_q_chunks(fic_rgb_ctx* c)
{
    const FicGeom& g = c->g;
    const int CT = fic_q_ct(g.B);
    const int nct = (int)(((long long)g.Nr * g.n_iso + 31) / 32);       // n_iso = 8: 8 columns per range block
    const SweepChunks k = q_chunks(c->q.ndtiles, (nct + CT - 1) / CT, 256LL * fic_q_resident(g.B), FIC_RGB_Q_MIN_TILES, fic_q_unroll(g.B, 1), c->opt_chunks);
    c->q.tiles_per_chunk = k.len;
    c->q.nchunks = k.nchunks;
}
// buffers of the matrix-core full search (same shapes as the grey q sweep)
int rgb_q_setup(fic_rgb_ctx* c)
{
    const FicGeom& g = c->g;
    FicRgbQ& q = c->q;
    if (q.amax) return FIC_OK;                           // the last one ensured: every store is there
    const int unroll = fic_q_unroll(g.B, 1), CT = fic_q_ct(g.B);
    const size_t NK = (size_t)g.n / 16;
    q.ndtiles = (g.Nd + 31) / 32;
    q.ndtiles_alloc = q.ndtiles + 2 * unroll;
    const int nct = (int)(((long long)g.Nr * g.n_iso + 31) / 32);       // n_iso = 8: 8 columns per range block
    q.nct_alloc = ((nct + CT - 1) / CT * CT + CT + 1) & ~1;
    // every store is ensured on its own pointer: a failed allocation leaves the earlier ones with the owner and is retried next time
    DevMem& m = c->mem;
    int rc = m.ensure(q.poolQ, (size_t)q.ndtiles_alloc * NK * 64 * 16);
    if (rc == FIC_OK) rc = m.ensure(q.dflat, (size_t)q.ndtiles_alloc * sizeof(uint32_t));
    if (rc == FIC_OK) rc = m.ensure(q.rngQ, (size_t)q.nct_alloc * NK * 64 * 16);
    if (rc == FIC_OK) rc = m.ensure(q.qst, (size_t)g.Nr * sizeof(FicRngStat));
    if (rc == FIC_OK) rc = m.ensure(q.rngE, (size_t)g.Nr * sizeof(float));
    if (rc == FIC_OK) rc = m.ensure(q.theta_g, (size_t)q.nct_alloc * 32 * sizeof(uint32_t));     // per column incl. the padded column tiles (the sweep's fast path reads them)
    if (rc == FIC_OK) rc = m.ensure(q.amax, sizeof(uint32_t));              // one word: the largest domain-operand norm
    return rc ? fail(FIC_E_HIP, "RGB matrix-core buffers: %s", g_mem_why) : FIC_OK;
}
}  // namespace

fic_rgb_ctx* fic_rgb_ctx_create(int device, int w, int h, int B, int wK, int planes)
{
    return fic_rgb_ctx_create_iso(device, w, h, B, wK, 1, planes);
}

fic_rgb_ctx* fic_rgb_ctx_create_iso(int device, int w, int h, int B, int wK, int n_iso, int planes)
{
    if (n_iso != 1 && n_iso != 8) { fail(FIC_E_ARGUMENT, "n_iso=%d: the joint-RGB path has 1 or 8 isometries", n_iso); return nullptr; }
    FicGeom g;
    if (make_geometry(w, h, B, wK, 1, planes, &g)) return nullptr;
    // the search key's low word carries c * 8 + k
    if (n_iso == 8 && (long long)g.wK * g.wK >= (1ll << 28)) {
        fail(FIC_E_GEOMETRY, "window of %d x %d candidates too large for 8 isometries (c * 8 + k must fit 31 bits)", g.wK, g.wK);
        return nullptr;
    }
    g.n_iso = n_iso;                 // the other fields are those of the 1-isometry geometry (the grey sweeps' tiling is not used here)
    if (!create_device_ok(device)) return nullptr;
    fic_rgb_ctx* c = new fic_rgb_ctx();
    c->device = device;
    c->mem.set_device(device);
    c->g = g;
    const size_t P = (size_t)planes, npix = (size_t)w * h, nr = (size_t)g.Nr, nd = (size_t)g.Nd, n = (size_t)g.n;
    DevMem& m = c->mem;
    int rc = FIC_OK;
    auto A = [&](int r) { if (rc == FIC_OK) rc = r; };
    A(m.alloc(c->scaled, P * g.Ws * g.Hs));
    A(m.alloc(c->pool_sum, P * nd * n));
    A(m.alloc(c->pool_st, P * nd));
    A(m.alloc(c->rng_t, P * nr * n));
    A(m.alloc(c->rng_st, P * nr));
    A(m.alloc(c->key, P * nr));
    A(m.alloc(c->idx_local, P * nr));
    A(m.alloc(c->idx_global, P * nr));
    A(m.alloc(c->a, P * nr));
    A(m.alloc(c->bR, P * nr));
    A(m.alloc(c->bG, P * nr));
    A(m.alloc(c->bB, P * nr));
    A(m.alloc(c->qrows, P * nr * 5));
    A(m.alloc(c->collage, P * npix));
    if (n_iso == 8) A(m.alloc(c->iso, P * nr));
    if (rc != FIC_OK) {
        delete c;
        return nullptr;
    }
    return c;
}

void fic_rgb_ctx_destroy(fic_rgb_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    delete c;
}

int fic_rgb_ctx_set_argb_host(fic_rgb_ctx* c, const int32_t* argb)
{
    if (!c || !argb) return fail(FIC_E_ARGUMENT, "fic_rgb_ctx_set_argb_host: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    if (int rc = upload_input(c, c->argb_own, argb, (size_t)c->g.planes * c->g.W * c->g.H)) return rc;
    c->argb = c->argb_own;
    return FIC_OK;
}

int fic_rgb_ctx_set_argb_device(fic_rgb_ctx* c, const void* dev_argb)
{
    if (!c || !dev_argb) return fail(FIC_E_ARGUMENT, "fic_rgb_ctx_set_argb_device: null argument");
    if (int rc = check_input_alignment("fic_rgb_ctx_set_argb_device", dev_argb, 4)) return rc;   // every kernel loads the pixels as int32_t, none wider
    std::lock_guard<std::mutex> lk(c->mu);
    c->argb = (const int32_t*)dev_argb;
    c->have_input = true;
    return FIC_OK;
}

int fic_rgb_ctx_encode(fic_rgb_ctx* c, int with_collage, void* hip_stream)
{
    if (!c) return fail(FIC_E_ARGUMENT, "fic_rgb_ctx_encode: null context");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->have_input) return fail(FIC_E_STATE, "fic_rgb_ctx_encode: no input image set");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)hip_stream;
    // scaled image, pool, stores, keys and outputs are shared with an earlier encode: on another stream the new work starts after it
    if (int rc = take_stream(c, s)) return rc;
    if (c->opt_search == 1) return rgb_lsq_encode(c, with_collage, s);      // least squares
    const FicGeom& g = c->g;
    // Full search: the matrix-core sweep where it pays (its prep costs ~50 us; the VALU sweep does ~1e11 pairs/s), or where
    // the VALU full-search kernel does not exist (B = 16).  FIC_RGB_SWEEP=1|2 / option "sweep" override.
    int want = c->opt_sweep;
    if (const char* env = getenv("FIC_RGB_SWEEP"))
        if (env[0] >= '1' && env[0] <= '2' && !env[1]) want = env[0] - '0';
    // 8 isometries: the same rule with 8 times the pairs (k_sweep_q<NK, 4>)
    const bool use_q = g.full && g.Nd < (1 << 24) && (want == 2 || (want == 0 && ((double)g.n_iso * g.Nr * g.Nd >= 3e7 || g.B == 16)));
    if (use_q && rgb_q_setup(c)) return FIC_E_HIP;
    if (use_q) rgb_q_chunks(c);
    if (!use_q && g.full && g.B <= 8) {                     // the VALU full-search sweep's f32 pool copy (k_sweep_rgb_fast), on first use
        const int rc = c->mem.ensure(c->pool_cf, (size_t)g.planes * g.Nd * g.n);
        if (rc != FIC_OK) return rc;
    }
    c->last_sweep = use_q ? 2 : 1;
    c->last_search = 0;
    {
        FicRgbBuffers b;                                  // image 0 of the batch: the kernels take the image from their grid
        FicRgbOutputs o;
        rgb_plane(c, 0, &b, &o);
        if (fic_launch_rgb_encode(b, o, with_collage ? c->collage : nullptr, g, s, use_q ? &c->q : nullptr))
            return fail(FIC_E_HIP, "RGB kernel launch failed");
    }
    c->encoded_any = true;
    c->have_collage = with_collage != 0;
    return FIC_OK;
}

int fic_rgb_ctx_set_option(fic_rgb_ctx* c, const char* name, int value)
{
    if (!c || !name) return fail(FIC_E_ARGUMENT, "fic_rgb_ctx_set_option: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!strcmp(name, "sweep")) {
        if (value < 0 || value > 2) return fail(FIC_E_ARGUMENT, "fic_rgb_ctx_set_option: sweep must be 0 (auto), 1 (VALU) or 2 (matrix cores)");
        c->opt_sweep = value;
        return FIC_OK;
    }
    // the core's options (fic_ctx_options.h).  Under "search" = 1 "sweep" means 0 (auto), 1 (generic), 2 (fast):
    // the same three values either way
    const int rc = set_core_option(c, kOptRgb, "fic_rgb_ctx_set_option: ", name, value);
    c->q.stats = c->sweep_stats;                       // the launchers' view of the "sweep_stats" counters
    return rc;
}

int fic_rgb_ctx_debug_q_host(fic_rgb_ctx* c, int which, void* out, int64_t capacity, int64_t* size)
{
    if (!c || !size) return fail(FIC_E_ARGUMENT, "fic_rgb_ctx_debug_q_host: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->encoded_any || c->last_sweep != 2 || !c->q.poolQ)
        return fail(FIC_E_STATE, "fic_rgb_ctx_debug_q_host: no encode through the matrix-core sweep (\"sweep\" = 2) yet");
    const FicRgbQ& q = c->q;
    const void* const stores[6] = {q.poolQ, q.dflat, q.rngQ, q.rngE, q.qst, q.amax};         // as of the last plane encoded
    return debug_store_host(c, "fic_rgb_ctx_debug_q_host", stores, 6, which, out, capacity, size);
}

int fic_rgb_ctx_last_sweep(fic_rgb_ctx* c)
{
    if (!c) return fail(FIC_E_ARGUMENT, "fic_rgb_ctx_last_sweep: null context");
    return c->last_sweep;
}

int fic_rgb_ctx_sweep_stats(fic_rgb_ctx* c, uint64_t* out8, int reset)
{
    if (!c || !out8) return fail(FIC_E_ARGUMENT, "fic_rgb_ctx_sweep_stats: null argument");
    return ctx_sweep_stats(c, "fic_rgb_ctx_sweep_stats", out8, reset);
}

int fic_rgb_ctx_last_kernel(fic_rgb_ctx* c, char* out, int capacity)
{
    if (!c || !out || capacity < 1) return fail(FIC_E_ARGUMENT, "fic_rgb_ctx_last_kernel: bad argument");
    const FicGeom& g = c->g;
    const int NK = g.n / 16;
    char buf[96];
    if (c->last_search == 1) {
        int NC = 1;
        fic_lsq_rgb_variant(g.B, g.n_iso, &NC);
        if (c->last_lsq_kind == 7) snprintf(buf, sizeof(buf), "k_sweep_lsq_rgb_q<%d, %d>", 3 * g.n / 16, g.n_iso == 8 ? 3 : 0);
        else if (c->last_lsq_kind == 2) snprintf(buf, sizeof(buf), "k_sweep_lsq_rgb_fast<%d, %d>", 3 * g.DW, NC);
        else snprintf(buf, sizeof(buf), "k_sweep_lsq_rgb_generic");
    } else if (c->last_sweep == 2) {
        const int kind = fic_q_multi_kind(c->q.nchunks, c->q.tiles_per_chunk);      // what fic_launch_rgbq instantiates
        const int mode = g.n_iso == 8 ? 4 : 3;
        if (kind == 2) snprintf(buf, sizeof(buf), "k_sweep_qs<%d, %d>", NK, mode);
        else snprintf(buf, sizeof(buf), "k_sweep_q<%d, %d, %s>", NK, mode, kind ? "true" : "false");
    } else if (c->last_sweep == 1) {
        const char* iso = g.n_iso == 8 ? "_iso" : "";
        if (g.full && g.B <= 8) snprintf(buf, sizeof(buf), "k_sweep_rgb_fast%s<%d>", iso, g.n);
        else snprintf(buf, sizeof(buf), "k_sweep_rgb%s", iso);
    } else snprintf(buf, sizeof(buf), "(none)");
    snprintf(out, (size_t)capacity, "%s", buf);
    return FIC_OK;
}

int fic_rgb_ctx_sync(fic_rgb_ctx* c)
{
    if (!c) return fail(FIC_E_ARGUMENT, "fic_rgb_ctx_sync: null context");
    return ctx_sync(c);
}

int fic_rgb_ctx_get_results_host(fic_rgb_ctx* c, int32_t* idx_local, float* a, float* bR, float* bG, float* bB, int32_t* qrows5,
                                 int32_t* collage_argb)
{
    if (!c) return fail(FIC_E_ARGUMENT, "fic_rgb_ctx_get_results_host: null context");
    if (!c->encoded_any) return fail(FIC_E_STATE, "fic_rgb_ctx_get_results_host: nothing encoded yet");
    if (collage_argb && !c->have_collage) return fail(FIC_E_STATE, "fic_rgb_ctx_get_results_host: the last encode built no collage");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->last_stream));
    const size_t n = (size_t)c->g.planes * c->g.Nr;
    if (idx_local) HIP_TRY(hipMemcpy(idx_local, c->idx_local, n * 4, hipMemcpyDeviceToHost));
    if (a) HIP_TRY(hipMemcpy(a, c->a, n * 4, hipMemcpyDeviceToHost));
    if (bR) HIP_TRY(hipMemcpy(bR, c->bR, n * 4, hipMemcpyDeviceToHost));
    if (bG) HIP_TRY(hipMemcpy(bG, c->bG, n * 4, hipMemcpyDeviceToHost));
    if (bB) HIP_TRY(hipMemcpy(bB, c->bB, n * 4, hipMemcpyDeviceToHost));
    if (qrows5) HIP_TRY(hipMemcpy(qrows5, c->qrows, n * 20, hipMemcpyDeviceToHost));
    if (collage_argb) HIP_TRY(hipMemcpy(collage_argb, c->collage, (size_t)c->g.planes * c->g.W * c->g.H * 4, hipMemcpyDeviceToHost));
    return FIC_OK;
}

int fic_rgb_ctx_get_iso_host(fic_rgb_ctx* c, int32_t* iso)
{
    if (!c || !iso) return fail(FIC_E_ARGUMENT, "fic_rgb_ctx_get_iso_host: null argument");
    if (!c->encoded_any) return fail(FIC_E_STATE, "fic_rgb_ctx_get_iso_host: nothing encoded yet");
    const size_t n = (size_t)c->g.planes * c->g.Nr;
    if (!c->iso) {                                     // n_iso = 1: the identity everywhere
        memset(iso, 0, n * sizeof(int32_t));
        return FIC_OK;
    }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->last_stream));
    HIP_TRY(hipMemcpy(iso, c->iso, n * 4, hipMemcpyDeviceToHost));
    return FIC_OK;
}

// decodeRGB (FC:430-508) from the context's quantised rows, plane by plane, everything device resident.  zoom = 1 runs in the
// context's own scratch; a zoomed decode takes an arena of the zoomed size (as fic_ctx_decode_zoom_host does).
int fic_rgb_ctx_decode_zoom_host(fic_rgb_ctx* c, int zoom, int32_t* argb_out, float* avg_error_out, int* iterations_out)
{
    if (!c || !argb_out) return fail(FIC_E_ARGUMENT, "fic_rgb_ctx_decode_zoom_host: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->encoded_any) return fail(FIC_E_STATE, "fic_rgb_ctx_decode_zoom_host: nothing encoded yet");
    const FicGeom& g = c->g;
    FicGeom g1 = g;
    if (zoom != 1) {
        const int rc = make_decode_geometry(g.W, g.H, g.B, g.wK, 1, 1, zoom, &g1);
        if (rc) return rc;
    }
    g1.planes = 1;
    HIP_TRY(hipSetDevice(c->device));
    const size_t npix = (size_t)g1.W * g1.H;
    DecodeJob J;
    if (zoom == 1) {
        if (int rc = c->mem.ensure(c->dec_image, npix)) return rc;
        if (int rc = c->mem.ensure(c->dec_scaled, (size_t)g.Ws * g.Hs)) return rc;
        if (int rc = c->mem.ensure(c->dec_state, 1)) return rc;
        if (int rc = c->mem.ensure(c->dec_sq, fic_decode_sq_words(1, npix))) return rc;
        J.borrow(kDecodeRgb, g1, c->last_stream, c->dec_scaled, c->dec_image, c->dec_state, c->dec_sq);
    } else {
        const int rc = J.open("fic_rgb_ctx_decode_zoom_host", c->device, kDecodeRgb, g1, c->last_stream);
        if (rc) return rc;
    }
    int rc = FIC_OK;
    for (int p = 0; p < g.planes && rc == FIC_OK; p++) {
        const int32_t* qrows = c->qrows + (size_t)p * g.Nr * 5;
        const int32_t* iso = c->iso ? c->iso + (size_t)p * g.Nr : nullptr;      // n_iso = 8: paint through src_k
        rc = J.run("fic_rgb_ctx_decode_zoom_host", nullptr, avg_error_out ? avg_error_out + p : nullptr,
                   iterations_out ? iterations_out + p : nullptr, nullptr, argb_out + (size_t)p * npix, [&](int counter) {
            return fic_launch_decode_iteration_rgb((int32_t*)J.scaled, (int32_t*)J.image, qrows, J.state, J.sq, counter, g1, J.stream, iso);
        });
        if (rc == FIC_E_ARGUMENT) rc = fail(rc, "%s (plane %d of the context)", std::string(g_err).c_str(), p);
    }
    return rc;
}

int fic_rgb_ctx_decode_host(fic_rgb_ctx* c, int32_t* argb_out, float* avg_error_out, int* iterations_out)
{
    return fic_rgb_ctx_decode_zoom_host(c, 1, argb_out, avg_error_out, iterations_out);
}

int fic_encode_rgb_argb(const int32_t* argb, int w, int h, int B, int wK, int device, int32_t* idx_local, float* a,
                        float* bR, float* bG, float* bB, int32_t* qrows5, int32_t* collage_argb)
{
    if (!argb || !idx_local || !a || !bR || !bG || !bB) return fail(FIC_E_ARGUMENT, "fic_encode_rgb_argb: null argument");
    return fic_encode_rgb_iso_argb(argb, w, h, B, wK, 1, device, idx_local, a, bR, bG, bB, nullptr, qrows5, collage_argb);
}

}  // extern "C"

// the one-shot joint-RGB encode behind fic_encode_rgb_iso_argb (search 0) and fic_encode_rgb_lsq_argb (search 1, with E)
static int rgb_oneshot(const char* entry, int search, const int32_t* argb, int w, int h, int B, int wK, int n_iso, int device, int32_t* idx_local,
                       float* a, float* bR, float* bG, float* bB, int32_t* iso, int32_t* qrows5, int32_t* collage_argb, int64_t* E)
{
    if (!argb || !idx_local || !a || !bR || !bG || !bB) return fail(FIC_E_ARGUMENT, "%s: null argument", entry);
    if (n_iso != 1 && n_iso != 8) return fail(FIC_E_ARGUMENT, "n_iso=%d: the joint-RGB path has 1 or 8 isometries", n_iso);
    // the GUI re-encodes the same image on every slider move (CTL:125-145): keep the last few working sets
    Lease<fic_rgb_ctx> L;
    int rc = L.open(device, w, h, B, wK, n_iso, search);
    if (rc == FIC_OK) rc = fic_rgb_ctx_set_argb_host(L.c, argb);
    if (rc == FIC_OK) rc = fic_rgb_ctx_encode(L.c, collage_argb ? 1 : 0, nullptr);
    if (rc == FIC_OK) rc = fic_rgb_ctx_get_results_host(L.c, idx_local, a, bR, bG, bB, qrows5, collage_argb);
    if (rc == FIC_OK && iso) rc = fic_rgb_ctx_get_iso_host(L.c, iso);
    if (rc == FIC_OK && E) rc = fic_rgb_ctx_get_lsq_error_host(L.c, E);
    return L.close(rc);
}

extern "C" {

int fic_encode_rgb_iso_argb(const int32_t* argb, int w, int h, int B, int wK, int n_iso, int device, int32_t* idx_local, float* a,
                            float* bR, float* bG, float* bB, int32_t* iso, int32_t* qrows5, int32_t* collage_argb)
{
    return rgb_oneshot("fic_encode_rgb_iso_argb", 0, argb, w, h, B, wK, n_iso, device, idx_local, a, bR, bG, bB, iso, qrows5, collage_argb, nullptr);
}

int fic_encode_rgb_lsq_argb(const int32_t* argb, int w, int h, int B, int wK, int n_iso, int device, int32_t* idx_local, float* a,
                            float* bR, float* bG, float* bB, int32_t* iso, int32_t* qrows5, int32_t* collage_argb, int64_t* E)
{
    return rgb_oneshot("fic_encode_rgb_lsq_argb", 1, argb, w, h, B, wK, n_iso, device, idx_local, a, bR, bG, bB, iso, qrows5, collage_argb, E);
}

}  // extern "C"
