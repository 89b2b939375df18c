// fic_capi_rgb.cpp -- C ABI, joint-RGB path: encodeRGB (FC:171-219) as one-shot entry and as batched device-resident
// contexts (fic_rgb_ctx_*), decodeRGB from a context's codebook (on the decode job of fic_capi_decode.cpp).  Host-side orchestration only.
#include "fic_internal.h"

using namespace ficd;

extern "C" {

// ---- joint-RGB encode (encodeRGB FC:171-219) -----------------------------------------------------
// A context owns the device working set of `planes` colour images of one geometry (config-5 style batches; the one-shot
// entry keeps a few single-image contexts).  The kernels take the image from their grid: a batch is one launch per stage on the
// caller's stream (only the matrix-core full search runs image by image).  The covariance sums stay sequential f32 in the reference's order (FC:781-792: they exceed 2^24).
struct fic_rgb_ctx {
    int device = 0;
    FicGeom g;
    int32_t* argb_own = nullptr;     // context-owned input copy
    const int32_t* argb = nullptr;   // input in use (own copy or the caller's device pointer)
    int32_t* scaled = nullptr;       // per plane: [H/2][W/2]
    uint16_t* pool_sum = nullptr;    // [N_d][n]
    float* pool_cf = nullptr;        // [N_d][n] (full search at B = 4 / 8)
    FicRgbDomStat* pool_st = nullptr;
    int16_t* rng_t = nullptr;
    FicRgbRngStat* rng_st = nullptr;
    unsigned long long* key = nullptr;
    int32_t *idx_local = nullptr, *idx_global = nullptr, *qrows = nullptr, *collage = nullptr;
    float *a = nullptr, *bR = nullptr, *bG = nullptr, *bB = nullptr;
    int32_t* iso = nullptr;          // winning isometries [planes][N_r] (n_iso = 8 contexts only; g.n_iso says which)
    int32_t* dec_image = nullptr;    // decoder: image, scaled image, state, per-pixel squared changes (one plane at a time)
    int32_t* dec_scaled = nullptr;
    FicDecodeState* dec_state = nullptr;
    uint32_t* dec_sq = nullptr;
    FicRgbQ q;                       // matrix-core full search (allocated on first use; one image at a time, stream-ordered)
    int opt_sweep = 0;               // 0 auto, 1 VALU sweeps, 2 matrix-core full search
    int opt_chunks = 0;              // pool chunks of the matrix-core sweep (0 = automatic)
    int last_sweep = 0;              // what the last encode ran: 1 / 2
    bool have_input = false, encoded_any = false, have_collage = false;
    hipStream_t last_stream = nullptr;
    std::mutex mu;
};

namespace {
void rgb_free_all(fic_rgb_ctx* c)
{
    (void)hipSetDevice(c->device);
    void* ptrs[] = {c->argb_own, c->scaled, c->pool_sum, c->pool_cf, c->pool_st, c->rng_t, c->rng_st, c->key, c->idx_local,
                    c->idx_global, c->qrows, c->collage, c->a, c->bR, c->bG, c->bB, c->iso, c->dec_image, c->dec_scaled, c->dec_state, c->dec_sq,
                    c->q.poolQ, c->q.dflat, c->q.rngQ, c->q.qst, c->q.rngE, c->q.theta_g, c->q.amax, c->q.stats};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
}
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
// pool chunks of the matrix-core full search: the policy of the grey q sweep (fic_capi.cpp, q_sweep), or the "chunks" option
void rgb_q_chunks(fic_rgb_ctx* c)
{
    const FicGeom& g = c->g;
    FicRgbQ& q = c->q;
    const int unroll = fic_q_unroll(g.B, 1), CT = fic_q_ct(g.B);
    const int nct = (int)(((long long)g.Nr * g.n_iso + 31) / 32);       // n_iso = 8: 8 columns per range block
    long long nc = c->opt_chunks;
    if (nc <= 0) {
        const long long base_wg = (nct + CT - 1) / CT;
        const long long resident = 256LL * fic_q_resident(g.B);
        auto ceil_div = [](long long a, long long b) { return (a + b - 1) / b; };
        long long fill = base_wg < resident ? ceil_div(2 * resident, base_wg) : 1;
        if (fill > q.ndtiles / 16) fill = q.ndtiles / 16;
        long long bal = ceil_div(8 * resident, base_wg);
        if (bal > q.ndtiles / 1024) bal = q.ndtiles / 1024;
        nc = fill > bal ? fill : bal;
    }
    if (nc < 1) nc = 1;
    if (nc > q.ndtiles) nc = q.ndtiles;
    int tpc = (int)((q.ndtiles + nc - 1) / nc);
    tpc = (tpc + unroll - 1) / unroll * unroll;
    q.tiles_per_chunk = tpc;
    q.nchunks = (q.ndtiles + tpc - 1) / tpc;
}
// buffers of the matrix-core full search (same shapes as the grey q sweep)
int rgb_q_setup(fic_rgb_ctx* c)
{
    const FicGeom& g = c->g;
    FicRgbQ& q = c->q;
    if (q.poolQ) return FIC_OK;
    unsigned long long* const stats = q.stats;           // option "sweep_stats": set before the first matrix-core encode too
    const int unroll = fic_q_unroll(g.B, 1), CT = fic_q_ct(g.B);
    const size_t NK = (size_t)g.n / 16;
    q.ndtiles = (g.Nd + 31) / 32;
    q.ndtiles_alloc = q.ndtiles + 2 * unroll;
    const int nct = (int)(((long long)g.Nr * g.n_iso + 31) / 32);       // n_iso = 8: 8 columns per range block
    q.nct_alloc = ((nct + CT - 1) / CT * CT + CT + 1) & ~1;
    int rc = FIC_OK;
    auto A = [&](hipError_t e) { if (rc == FIC_OK && e != hipSuccess) rc = fail(FIC_E_HIP, "RGB matrix-core buffers: %s", hipGetErrorString(e)); };
    A(hipMalloc(&q.poolQ, (size_t)q.ndtiles_alloc * NK * 64 * 16));
    A(hipMalloc(&q.dflat, (size_t)q.ndtiles_alloc * sizeof(uint32_t)));
    A(hipMalloc(&q.rngQ, (size_t)q.nct_alloc * NK * 64 * 16));
    A(hipMalloc(&q.qst, (size_t)g.Nr * sizeof(FicRngStat)));
    A(hipMalloc(&q.rngE, (size_t)g.Nr * sizeof(float)));
    A(hipMalloc(&q.theta_g, (size_t)q.nct_alloc * 32 * sizeof(uint32_t)));     // per column incl. the padded column tiles (the sweep's fast path reads them)
    A(hipMalloc(&q.amax, 256));
    if (rc != FIC_OK) {
        void* ptrs[] = {q.poolQ, q.dflat, q.rngQ, q.qst, q.rngE, q.theta_g, q.amax};
        for (void* p : ptrs)
            if (p) (void)hipFree(p);
        q = FicRgbQ();
        q.stats = stats;
    }
    return rc;
}
// idle single-image contexts of the one-shot RGB entry, most recently used last
std::mutex g_rgb_mu;
std::vector<fic_rgb_ctx*> g_rgb_cache;
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
    int ndev = fic_device_count();
    if (ndev <= 0) { fail(FIC_E_NO_DEVICE, "no HIP device visible (this library has no CPU path)"); return nullptr; }
    if (device < 0 || device >= ndev) { fail(FIC_E_NO_DEVICE, "device %d out of range (0..%d)", device, ndev - 1); return nullptr; }
    if (hipSetDevice(device) != hipSuccess) { fail(FIC_E_HIP, "hipSetDevice(%d) failed", device); return nullptr; }
    fic_rgb_ctx* c = new fic_rgb_ctx();
    c->device = device;
    c->g = g;
    const size_t P = (size_t)planes, npix = (size_t)w * h, nr = (size_t)g.Nr, nd = (size_t)g.Nd, n = (size_t)g.n;
    int rc = FIC_OK;
    auto A = [&](int r) { if (rc == FIC_OK) rc = r; };
    A(dev_alloc(&c->scaled, P * g.Ws * g.Hs));
    A(dev_alloc(&c->pool_sum, P * nd * n));
    A(dev_alloc(&c->pool_st, P * nd));
    A(dev_alloc(&c->rng_t, P * nr * n));
    A(dev_alloc(&c->rng_st, P * nr));
    A(dev_alloc(&c->key, P * nr));
    A(dev_alloc(&c->idx_local, P * nr));
    A(dev_alloc(&c->idx_global, P * nr));
    A(dev_alloc(&c->a, P * nr));
    A(dev_alloc(&c->bR, P * nr));
    A(dev_alloc(&c->bG, P * nr));
    A(dev_alloc(&c->bB, P * nr));
    A(dev_alloc(&c->qrows, P * nr * 5));
    A(dev_alloc(&c->collage, P * npix));
    if (n_iso == 8) A(dev_alloc(&c->iso, P * nr));
    if (rc != FIC_OK) {
        rgb_free_all(c);
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
    rgb_free_all(c);
    delete c;
}

int fic_rgb_ctx_set_argb_host(fic_rgb_ctx* c, const int32_t* argb)
{
    if (!c || !argb) return fail(FIC_E_ARGUMENT, "fic_rgb_ctx_set_argb_host: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    const size_t npix = (size_t)c->g.planes * c->g.W * c->g.H;
    if (!c->argb_own) { int rc = dev_alloc(&c->argb_own, npix); if (rc) return rc; }
    HIP_TRY(hipStreamSynchronize(c->last_stream));     // a previous encode may still read the copy
    HIP_TRY(hipMemcpy(c->argb_own, argb, npix * sizeof(int32_t), hipMemcpyHostToDevice));
    c->argb = c->argb_own;
    c->have_input = true;
    return FIC_OK;
}

int fic_rgb_ctx_set_argb_device(fic_rgb_ctx* c, const void* dev_argb)
{
    if (!c || !dev_argb) return fail(FIC_E_ARGUMENT, "fic_rgb_ctx_set_argb_device: null argument");
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
    c->last_stream = s;
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
    if (!use_q && g.full && g.B <= 8 && !c->pool_cf) {      // the VALU full-search sweep's f32 pool copy (k_sweep_rgb_fast), on first use
        const int rc = dev_alloc(&c->pool_cf, (size_t)g.planes * g.Nd * g.n);
        if (rc != FIC_OK) return rc;
    }
    c->last_sweep = use_q ? 2 : 1;
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
    if (!strcmp(name, "chunks")) {
        if (value < 0) return fail(FIC_E_ARGUMENT, "fic_rgb_ctx_set_option: chunks must be >= 0");
        c->opt_chunks = value;
        return FIC_OK;
    }
    if (!strcmp(name, "q_eshift")) {                   // diagnostic: the matrix-core sweep's E_r times 2^-value (> 0: WRONG codebooks)
        if (value < -12 || value > 4) return fail(FIC_E_ARGUMENT, "fic_rgb_ctx_set_option: q_eshift must be in -12..4");
        c->g.q_eshift = value;
        return FIC_OK;
    }
    if (!strcmp(name, "sweep_stats")) {                // test hook: counters of the matrix-core sweep (fic_rgb_ctx_sweep_stats)
        HIP_TRY(hipSetDevice(c->device));
        if (value && !c->q.stats) {
            HIP_TRY(hipMalloc((void**)&c->q.stats, 8 * sizeof(unsigned long long)));
            HIP_TRY(hipMemset(c->q.stats, 0, 8 * sizeof(unsigned long long)));
            HIP_TRY(hipStreamSynchronize(nullptr));            // the fill is only enqueued (null stream); sweeps run on other streams
        } else if (!value && c->q.stats) {
            HIP_TRY(hipStreamSynchronize(c->last_stream));
            (void)hipFree(c->q.stats);
            c->q.stats = nullptr;
        }
        return FIC_OK;
    }
    return fail(FIC_E_ARGUMENT, "fic_rgb_ctx_set_option: unknown option '%s'", name);
}

int fic_rgb_ctx_debug_q_host(fic_rgb_ctx* c, int which, void* out, int64_t capacity, int64_t* size)
{
    if (!c || !size) return fail(FIC_E_ARGUMENT, "fic_rgb_ctx_debug_q_host: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->encoded_any || c->last_sweep != 2 || !c->q.poolQ)
        return fail(FIC_E_STATE, "fic_rgb_ctx_debug_q_host: no encode through the matrix-core sweep (\"sweep\" = 2) yet");
    const FicGeom& g = c->g;
    const FicRgbQ& q = c->q;
    const size_t NK = (size_t)g.n / 16;
    const void* src = nullptr;
    size_t bytes = 0;
    switch (which) {                                   // the stores exactly as rgb_q_setup allocates them (last plane encoded)
    case 0: src = q.poolQ; bytes = (size_t)q.ndtiles_alloc * NK * 64 * 16; break;
    case 1: src = q.dflat; bytes = (size_t)q.ndtiles_alloc * sizeof(uint32_t); break;
    case 2: src = q.rngQ; bytes = (size_t)q.nct_alloc * NK * 64 * 16; break;
    case 3: src = q.rngE; bytes = (size_t)g.Nr * sizeof(float); break;
    case 4: src = q.qst; bytes = (size_t)g.Nr * sizeof(FicRngStat); break;
    case 5: src = q.amax; bytes = sizeof(uint32_t); break;
    default: return fail(FIC_E_ARGUMENT, "fic_rgb_ctx_debug_q_host: which must be 0..5");
    }
    *size = (int64_t)bytes;
    if (!out) return FIC_OK;
    if (capacity < (int64_t)bytes) return fail(FIC_E_CAPACITY, "fic_rgb_ctx_debug_q_host: %zu bytes needed", bytes);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->last_stream));
    HIP_TRY(hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost));
    return FIC_OK;
}

int fic_rgb_ctx_last_sweep(fic_rgb_ctx* c)
{
    if (!c) return fail(FIC_E_ARGUMENT, "fic_rgb_ctx_last_sweep: null context");
    return c->last_sweep;
}

int fic_rgb_ctx_sweep_stats(fic_rgb_ctx* c, uint64_t* out8, int reset)
{
    if (!c || !out8) return fail(FIC_E_ARGUMENT, "fic_rgb_ctx_sweep_stats: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->q.stats) return fail(FIC_E_STATE, "fic_rgb_ctx_sweep_stats: set the option \"sweep_stats\" first");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->last_stream));
    HIP_TRY(hipMemcpy(out8, c->q.stats, 8 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (reset) {
        HIP_TRY(hipMemset(c->q.stats, 0, 8 * sizeof(uint64_t)));
        HIP_TRY(hipStreamSynchronize(nullptr));
    }
    return FIC_OK;
}

int fic_rgb_ctx_last_kernel(fic_rgb_ctx* c, char* out, int capacity)
{
    if (!c || !out || capacity < 1) return fail(FIC_E_ARGUMENT, "fic_rgb_ctx_last_kernel: bad argument");
    const FicGeom& g = c->g;
    const int NK = g.n / 16;
    char buf[96];
    if (c->last_sweep == 2) {
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
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->last_stream));
    return FIC_OK;
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
        if (!c->dec_image) { int rc = dev_alloc(&c->dec_image, npix); if (rc) return rc; }
        if (!c->dec_scaled) { int rc = dev_alloc(&c->dec_scaled, (size_t)g.Ws * g.Hs); if (rc) return rc; }
        if (!c->dec_state) { int rc = dev_alloc(&c->dec_state, 1); if (rc) return rc; }
        if (!c->dec_sq) { int rc = dev_alloc(&c->dec_sq, fic_decode_sq_words(1, npix)); if (rc) return rc; }
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

}  // extern "C"

fic_rgb_ctx* ficd::rgb_cache_take(int device, int w, int h, int B, int wK, int n_iso)
{
    std::lock_guard<std::mutex> lk(g_rgb_mu);
    for (size_t i = g_rgb_cache.size(); i-- > 0;) {
        fic_rgb_ctx* c = g_rgb_cache[i];
        const FicGeom& g = c->g;
        if (c->device == device && g.W == w && g.H == h && g.B == B && g.wK == wK && g.n_iso == n_iso && g.planes == 1) {
            g_rgb_cache.erase(g_rgb_cache.begin() + (long)i);
            return c;
        }
    }
    return nullptr;
}
void ficd::rgb_cache_give(fic_rgb_ctx* c)
{
    fic_rgb_ctx* evict = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_rgb_mu);
        g_rgb_cache.push_back(c);
        if (g_rgb_cache.size() > 4) {
            evict = g_rgb_cache.front();
            g_rgb_cache.erase(g_rgb_cache.begin());
        }
    }
    if (evict) fic_rgb_ctx_destroy(evict);
}

void ficd::rgb_ctx_views(const fic_rgb_ctx* c, const int32_t** argb, const int32_t** scaled, const int32_t** qrows5, const int32_t** iso)
{
    if (iso) *iso = c->iso;
    if (argb) *argb = c->argb;
    if (scaled) *scaled = c->scaled;
    if (qrows5) *qrows5 = c->qrows;
}

extern "C" {

int fic_encode_rgb_argb(const int32_t* argb, int w, int h, int B, int wK, int device, int32_t* idx_local, float* a,
                        float* bR, float* bG, float* bB, int32_t* qrows5, int32_t* collage_argb)
{
    if (!argb || !idx_local || !a || !bR || !bG || !bB) return fail(FIC_E_ARGUMENT, "fic_encode_rgb_argb: null argument");
    return fic_encode_rgb_iso_argb(argb, w, h, B, wK, 1, device, idx_local, a, bR, bG, bB, nullptr, qrows5, collage_argb);
}

int fic_encode_rgb_iso_argb(const int32_t* argb, int w, int h, int B, int wK, int n_iso, int device, int32_t* idx_local, float* a,
                            float* bR, float* bG, float* bB, int32_t* iso, int32_t* qrows5, int32_t* collage_argb)
{
    if (!argb || !idx_local || !a || !bR || !bG || !bB) return fail(FIC_E_ARGUMENT, "fic_encode_rgb_iso_argb: null argument");
    if (n_iso != 1 && n_iso != 8) return fail(FIC_E_ARGUMENT, "n_iso=%d: the joint-RGB path has 1 or 8 isometries", n_iso);
    // the GUI re-encodes the same image on every slider move (CTL:125-145): keep the last few working sets
    fic_rgb_ctx* c = rgb_cache_take(device, w, h, B, wK, n_iso);
    if (!c) c = fic_rgb_ctx_create_iso(device, w, h, B, wK, n_iso, 1);
    if (!c) return g_err_code ? g_err_code : FIC_E_HIP;   // fic_rgb_ctx_create recorded why
    int rc = fic_rgb_ctx_set_argb_host(c, argb);
    if (rc == FIC_OK) rc = fic_rgb_ctx_encode(c, collage_argb ? 1 : 0, nullptr);
    if (rc == FIC_OK) rc = fic_rgb_ctx_get_results_host(c, idx_local, a, bR, bG, bB, qrows5, collage_argb);
    if (rc == FIC_OK && iso) rc = fic_rgb_ctx_get_iso_host(c, iso);
    ErrKeep keep;
    if (rc == FIC_OK) rgb_cache_give(c);
    else fic_rgb_ctx_destroy(c);
    return rc;
}

}  // extern "C"

void ficd::release_rgb_cache()
{
    std::vector<fic_rgb_ctx*> drop;
    {
        std::lock_guard<std::mutex> lk(g_rgb_mu);
        drop.swap(g_rgb_cache);
    }
    for (fic_rgb_ctx* c : drop) fic_rgb_ctx_destroy(c);
}
