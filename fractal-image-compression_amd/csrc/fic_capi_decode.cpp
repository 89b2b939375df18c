// fic_capi_decode.cpp -- C ABI, decoder entries: FractalCompression.decode on .run streams (FC:547-553 -> decodeGreyScale
// FC:356-421, decodeRGB FC:430-508), the decode of a context's own codebook, and the fixed-B streams with an isometry column
// (tags 4 and 5: writers and decoders).  Host-side orchestration only.
#include "fic_internal.h"

using namespace ficd;

// ---- decoder (decodeGreyScale FC:356-421) ------------------------------------------------------
namespace {
// Device arenas of the stream decoders (struct Arena, fic_internal.h), kept between calls (the GUI decodes after every
// encode, CTL:178-179): one allocation per (device, size class) instead of four hipMalloc/hipFree per call.
// fic_release_cache() frees them.
std::mutex g_arena_mu;
std::vector<Arena> g_arenas;
constexpr size_t kArenaSlots = 4;

}  // namespace

int ficd::arena_take(int device, size_t bytes, Arena* out)
{
    {
        std::lock_guard<std::mutex> lk(g_arena_mu);
        for (size_t i = g_arenas.size(); i-- > 0;)
            if (g_arenas[i].device == device && g_arenas[i].bytes >= bytes && g_arenas[i].bytes <= 2 * bytes + (1u << 20)) {
                *out = g_arenas[i];
                g_arenas.erase(g_arenas.begin() + (long)i);
                return FIC_OK;
            }
    }
    out->device = device;
    out->bytes = bytes;
    HIP_TRY(hipMalloc((void**)&out->base, bytes));
    return FIC_OK;
}
void ficd::arena_give(const Arena& a)
{
    Arena evict;
    {
        std::lock_guard<std::mutex> lk(g_arena_mu);
        g_arenas.push_back(a);
        if (g_arenas.size() <= kArenaSlots) return;
        evict = g_arenas.front();
        g_arenas.erase(g_arenas.begin());
    }
    (void)hipSetDevice(evict.device);
    (void)hipFree(evict.base);
}

void ficd::release_decoder_arenas()
{
    std::vector<Arena> drop;
    {
        std::lock_guard<std::mutex> lk(g_arena_mu);
        drop.swap(g_arenas);
    }
    for (const Arena& a : drop) { (void)hipSetDevice(a.device); (void)hipFree(a.base); }
}

static thread_local int g_last_sum_fallbacks = 0;

// Runs the reconstruction loop on the device.  The first 8 iterations are enqueued in one go, later ones in pairs, and the
// per-plane loop state is read back after each group (a converging decode takes 6-9 iterations): one host sync per
// group, none per iteration; iterations enqueued behind the last one exit at once.  `iteration(counter)` enqueues one
// iteration (scale, paint, loop control) on s; d_image [planes][npix] pixels of kind.px_bytes is filled with kind.px_start here.
//   d_state [planes]: scratch of the caller
int ficd::decode_loop(const DecodeKind& kind, int planes, size_t npix, void* d_image, FicDecodeState* d_state, const float* avg_in,
                      float* avg_out, int* iters_out, int* seq_out, hipStream_t s, const std::function<int(int)>& iteration)
{
    const size_t P = (size_t)planes;
    std::vector<FicDecodeState> st(P);
    memset(st.data(), 0, P * sizeof(FicDecodeState));
    for (size_t p = 0; p < P; p++) st[p].avg = avg_in ? avg_in[p] : 0.0f;   // static avgError is never reset (FC:20)
    int rc = FIC_OK;
    hipError_t e = hipMemcpyAsync(d_state, st.data(), P * sizeof(FicDecodeState), hipMemcpyHostToDevice, s);
    if (e == hipSuccess)                                                            // generateGrayImage FC:1142-1148
        e = kind.px_bytes == 1 ? hipMemsetAsync(d_image, (int)kind.px_start, P * npix, s)
                               : hipMemsetD32Async((hipDeviceptr_t)d_image, (int)kind.px_start, P * npix, s);
    if (e != hipSuccess) rc = fail(FIC_E_HIP, "%s init: %s", kind.name, hipGetErrorString(e));
    for (int counter = 0; rc == FIC_OK && counter < 50; counter++) {
        if (iteration(counter)) {
            rc = fail(FIC_E_HIP, "%s iteration launch failed", kind.name);
            break;
        }
        // a converging decode takes 6-9 iterations: look at the loop state after 8, then after every second iteration
        if (counter == 7 || (counter > 7 && (counter & 1)) || counter == 49) {
            e = hipMemcpyAsync(st.data(), d_state, P * sizeof(FicDecodeState), hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) { rc = fail(FIC_E_HIP, "%s readback: %s", kind.name, hipGetErrorString(e)); break; }
            bool all = true;
            for (size_t p = 0; p < P; p++) all = all && st[p].done;
            if (all) break;
        }
    }
    if (rc != FIC_OK) return rc;
    for (size_t p = 0; p < P; p++) {
        if (st[p].bad_index) {
            const std::string of_plane = P > 1 ? " of plane " + std::to_string(p) : "";
            return fail(FIC_E_ARGUMENT, "%s: a codebook row%s points outside the domain pool (ArrayIndexOutOfBounds at %s in the "
                                        "reference)", kind.name, of_plane.c_str(), kind.paint_line);
        }
        if (avg_out) avg_out[p] = st[p].avg_out;
        if (iters_out) iters_out[p] = st[p].iters;
        if (seq_out) seq_out[p] = st[p].seq_sums;
    }
    return FIC_OK;
}

extern "C" {

//   d_state [planes], d_sqbuf u32 [planes][W*H]: scratch of the caller
static int run_decode_loop(const FicGeom& g, uint8_t* d_scaled, uint8_t* d_image, const int32_t* d_qrows,
                           const int32_t* d_iso, FicDecodeState* d_state, uint32_t* d_sqbuf, const float* avg_in,
                           float* avg_out, int* iters_out, int* seq_out, hipStream_t s)
{
    return decode_loop(kDecodeGrey, g.planes, (size_t)g.W * g.H, d_image, d_state, avg_in, avg_out, iters_out, seq_out, s, [&](int counter) {
        return fic_launch_decode_iteration(d_scaled, d_image, d_qrows, d_iso, d_state, d_sqbuf, counter, g, s);
    });
}

int fic_ctx_decode_zoom_host(fic_ctx* c, int zoom, uint8_t* gray_out, float* avg_error_out, int* iterations_out)
{
    if (!c || !gray_out) return fail(FIC_E_ARGUMENT, "fic_ctx_decode_host: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->encoded_any) return fail(FIC_E_STATE, "fic_ctx_decode_host: nothing encoded yet");
    const int32_t* d_iso = c->g.n_iso > 1 ? c->o.iso : nullptr;
    if (zoom != 1) {
        // the context's own scratch holds the encoded size: a zoomed decode takes an arena of the zoomed size instead
        FicGeom g;
        int rc = make_decode_geometry(c->g.W, c->g.H, c->g.B, c->g.wK, c->g.n_iso, c->g.planes, zoom, &g);
        if (rc) return rc;
        HIP_TRY(hipSetDevice(c->device));
        const size_t P = (size_t)g.planes, npix = P * g.W * g.H;
        const size_t o_scaled = 0, o_image = o_scaled + align256(P * g.Ws * g.Hs), o_state = o_image + align256(npix),
                     o_sq = o_state + align256(P * sizeof(FicDecodeState)),
                     total = o_sq + align256(fic_decode_sq_words(P, (size_t)g.W * g.H) * 4);
        Arena ar;
        rc = arena_take(c->device, total, &ar);
        if (rc) return rc;
        hipError_t e = hipStreamSynchronize(c->last_stream);
        if (e != hipSuccess) rc = fail(FIC_E_HIP, "fic_ctx_decode_zoom_host: %s", hipGetErrorString(e));
        if (rc == FIC_OK)
            rc = run_decode_loop(g, (uint8_t*)(ar.base + o_scaled), (uint8_t*)(ar.base + o_image), c->o.qrows, d_iso,
                                 (FicDecodeState*)(ar.base + o_state), (uint32_t*)(ar.base + o_sq), nullptr, avg_error_out, iterations_out,
                                 nullptr, c->last_stream);
        if (rc == FIC_OK) {
            e = hipMemcpy(gray_out, ar.base + o_image, npix, hipMemcpyDeviceToHost);
            if (e != hipSuccess) rc = fail(FIC_E_HIP, "fic_ctx_decode_zoom_host: %s", hipGetErrorString(e));
        }
        arena_give(ar);
        return rc;
    }
    HIP_TRY(hipSetDevice(c->device));
    const FicGeom& g = c->g;
    size_t npix = (size_t)g.planes * g.W * g.H;
    if (!c->decoded) { int rc = dev_alloc(&c->decoded, npix); if (rc) return rc; }
    if (!c->dec_state) { int rc = dev_alloc(&c->dec_state, (size_t)g.planes); if (rc) return rc; }
    if (!c->dec_sq) { int rc = dev_alloc(&c->dec_sq, fic_decode_sq_words((size_t)g.planes, (size_t)g.W * g.H)); if (rc) return rc; }
    HIP_TRY(hipStreamSynchronize(c->last_stream));
    int rc = run_decode_loop(g, c->b.scaled, c->decoded, c->o.qrows, d_iso, c->dec_state, c->dec_sq,
                             nullptr, avg_error_out, iterations_out, nullptr, c->last_stream);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(gray_out, c->decoded, npix, hipMemcpyDeviceToHost));
    return FIC_OK;
}

int fic_ctx_decode_host(fic_ctx* c, uint8_t* gray_out, float* avg_error_out, int* iterations_out)
{
    return fic_ctx_decode_zoom_host(c, 1, gray_out, avg_error_out, iterations_out);
}

// The header's geometry (w, h, B, wK) must be one the encoders take; the decode runs on it times `zoom` (make_decode_geometry).
static int decode_gray_run_impl(const uint8_t* run, int64_t len, int zoom, int device, uint8_t* gray_out, int64_t capacity, int* w_out,
                                int* h_out, float* avg_error_io, int* iterations, int* seq_sums)
{
    if (!run || len < 20) return fail(FIC_E_ARGUMENT, "fic_decode_gray_run: stream shorter than the 20-byte header");
    if (get_be32(run) != 0)
        return fail(FIC_E_NOT_GREY, "fic_decode_gray_run: isRGB = %d (FC:548-552 dispatches to decodeRGB)", get_be32(run));
    const int w0 = get_be32(run + 4), h0 = get_be32(run + 8), B = get_be32(run + 12), wK = get_be32(run + 16);
    FicGeom g;
    int rc = make_geometry(w0, h0, B, wK, 1, 1, &g);
    if (rc == FIC_OK) rc = make_decode_geometry(w0, h0, B, wK, 1, 1, zoom, &g);
    if (rc) return rc;
    const int w = g.W, h = g.H;
    if (w_out) *w_out = w;
    if (h_out) *h_out = h;
    if (len < 20 + 12 * (int64_t)g.Nr)
        return fail(FIC_E_ARGUMENT, "fic_decode_gray_run: %lld bytes, need %lld (EOFException in the reference)",
                    (long long)len, (long long)(20 + 12 * (int64_t)g.Nr));
    if (!gray_out || capacity < (int64_t)w * h) return fail(FIC_E_CAPACITY, "fic_decode_gray_run: output needs %d bytes", w * h);
    rc = check_device(device);
    if (rc) return rc;
    std::vector<int32_t> q((size_t)g.Nr * 3);
    for (size_t i = 0; i < q.size(); i++) q[i] = get_be32(run + 20 + 4 * i);          // FC:372-374
    const size_t npix = (size_t)w * h;
    const size_t o_scaled = 0, o_image = o_scaled + align256((size_t)g.Ws * g.Hs), o_q = o_image + align256(npix),
                 o_state = o_q + align256(q.size() * 4), o_sq = o_state + align256(sizeof(FicDecodeState)),
                 total = o_sq + align256(fic_decode_sq_words(1, npix) * 4);
    Arena ar;
    rc = arena_take(device, total, &ar);
    if (rc) return rc;
    hipError_t e = hipMemcpy(ar.base + o_q, q.data(), q.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) rc = fail(FIC_E_HIP, "fic_decode_gray_run: %s", hipGetErrorString(e));
    float avg = avg_error_io ? *avg_error_io : 0.0f;
    if (rc == FIC_OK)
        rc = run_decode_loop(g, (uint8_t*)(ar.base + o_scaled), (uint8_t*)(ar.base + o_image), (const int32_t*)(ar.base + o_q), nullptr,
                             (FicDecodeState*)(ar.base + o_state), (uint32_t*)(ar.base + o_sq), &avg, &avg, iterations, seq_sums, nullptr);
    if (rc == FIC_OK) {
        e = hipMemcpy(gray_out, ar.base + o_image, npix, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(FIC_E_HIP, "fic_decode_gray_run: %s", hipGetErrorString(e));
    }
    if (rc == FIC_OK && avg_error_io) *avg_error_io = avg;
    arena_give(ar);
    return rc;
}

int fic_decode_gray_run_zoom(const uint8_t* run, int64_t len, int zoom, int device, uint8_t* gray_out, int64_t capacity, int* w_out,
                             int* h_out, float* avg_error_io, int* iterations)
{
    return decode_gray_run_impl(run, len, zoom, device, gray_out, capacity, w_out, h_out, avg_error_io, iterations, nullptr);
}

int fic_decode_gray_run(const uint8_t* run, int64_t len, int device, uint8_t* gray_out, int64_t capacity, int* w_out,
                        int* h_out, float* avg_error_io, int* iterations)
{
    return fic_decode_gray_run_zoom(run, len, 1, device, gray_out, capacity, w_out, h_out, avg_error_io, iterations);
}

// Test hook: the decoder's reproduction of Java's `avgError += (float) v[i]` loop (FC:407) on arbitrary values.
int fic_debug_float_sum(int device, float carry, const uint32_t* vals, int count, float* out)
{
    if (!vals || !out || count < 0) return fail(FIC_E_ARGUMENT, "fic_debug_float_sum: bad argument");
    int rc = check_device(device);
    if (rc) return rc;
    uint32_t* d = nullptr;
    float* r = nullptr;
    uint32_t* maps = nullptr;
    HIP_TRY(hipMalloc((void**)&d, (size_t)(count + 4) * 4));
    hipError_t e = hipMalloc((void**)&r, 8);
    if (e == hipSuccess) e = hipMalloc((void**)&maps, (fic_float_sum_map_words((size_t)count) + 4) * 4);
    if (e == hipSuccess) e = hipMemcpy(d, vals, (size_t)count * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) rc = fail(FIC_E_HIP, "fic_debug_float_sum: %s", hipGetErrorString(e));
    if (rc == FIC_OK && fic_launch_float_sum_probe(carry, d, count, maps, r, nullptr)) rc = fail(FIC_E_HIP, "k_float_sum_probe launch failed");
    if (rc == FIC_OK) {
        float two[2] = {0.0f, 0.0f};
        e = hipMemcpy(two, r, 8, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(FIC_E_HIP, "fic_debug_float_sum: %s", hipGetErrorString(e));
        out[0] = two[0];
        g_last_sum_fallbacks = (int)two[1];
    }
    (void)hipFree(d);
    if (r) (void)hipFree(r);
    if (maps) (void)hipFree(maps);
    return rc;
}

// Test hook: segments of the last fic_debug_float_sum on this thread that went through the sequential-order path.
int fic_debug_float_sum_fallbacks(void) { return g_last_sum_fallbacks; }

// Test hook: fic_decode_gray_run that also reports how many iterations needed the sequential (Java-order) float sum.
int fic_debug_decode_gray_run(const uint8_t* run, int64_t len, int device, uint8_t* gray_out, int64_t capacity,
                              float* avg_error_io, int* iterations, int* seq_sums)
{
    return decode_gray_run_impl(run, len, 1, device, gray_out, capacity, nullptr, nullptr, avg_error_io, iterations, seq_sums);
}

// ---- decodeRGB (FC:430-508) -----------------------------------------------------------------------
int fic_decode_rgb_run_zoom(const uint8_t* run, int64_t len, int zoom, int device, int32_t* argb_out, int64_t capacity_pixels,
                            int* w_out, int* h_out, float* avg_error_io, int* iterations)
{
    if (!run || len < 20) return fail(FIC_E_ARGUMENT, "fic_decode_rgb_run: stream shorter than the 20-byte header");
    if (get_be32(run) == 0) return fail(FIC_E_ARGUMENT, "fic_decode_rgb_run: isRGB = 0 (FC:548-550 dispatches to decodeGreyScale)");
    const int w0 = get_be32(run + 4), h0 = get_be32(run + 8), B = get_be32(run + 12), wK = get_be32(run + 16);
    FicGeom g;
    int rc = make_geometry(w0, h0, B, wK, 1, 1, &g);
    if (rc == FIC_OK) rc = make_decode_geometry(w0, h0, B, wK, 1, 1, zoom, &g);
    if (rc) return rc;
    const int w = g.W, h = g.H;
    if (w_out) *w_out = w;
    if (h_out) *h_out = h;
    if (len < 20 + 20 * (int64_t)g.Nr)
        return fail(FIC_E_ARGUMENT, "fic_decode_rgb_run: %lld bytes, need %lld (EOFException in the reference)",
                    (long long)len, (long long)(20 + 20 * (int64_t)g.Nr));
    if (!argb_out || capacity_pixels < (int64_t)w * h) return fail(FIC_E_CAPACITY, "fic_decode_rgb_run: output needs %d ints", w * h);
    rc = check_device(device);
    if (rc) return rc;
    std::vector<int32_t> q((size_t)g.Nr * 5);
    for (size_t i = 0; i < q.size(); i++) q[i] = get_be32(run + 20 + 4 * i);          // FC:446-450
    const size_t npix = (size_t)w * h;
    const size_t o_scaled = 0, o_image = o_scaled + align256((size_t)g.Ws * g.Hs * 4), o_q = o_image + align256(npix * 4),
                 o_state = o_q + align256(q.size() * 4), o_sq = o_state + align256(sizeof(FicDecodeState)),
                 total = o_sq + align256(fic_decode_sq_words(1, npix) * 4);
    Arena ar;
    rc = arena_take(device, total, &ar);
    if (rc) return rc;
    int32_t* d_scaled = (int32_t*)(ar.base + o_scaled);
    int32_t* d_image = (int32_t*)(ar.base + o_image);
    int32_t* d_q = (int32_t*)(ar.base + o_q);
    FicDecodeState* d_state = (FicDecodeState*)(ar.base + o_state);
    uint32_t* d_sq = (uint32_t*)(ar.base + o_sq);
    hipError_t e = hipMemcpy(d_q, q.data(), q.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) rc = fail(FIC_E_HIP, "fic_decode_rgb_run: %s", hipGetErrorString(e));
    float avg = avg_error_io ? *avg_error_io : 0.0f;
    if (rc == FIC_OK)
        rc = decode_loop(kDecodeRgb, 1, npix, d_image, d_state, &avg, &avg, iterations, nullptr, nullptr, [&](int counter) {
            return fic_launch_decode_iteration_rgb(d_scaled, d_image, d_q, d_state, d_sq, counter, g, nullptr);
        });
    if (rc == FIC_OK) {
        e = hipMemcpy(argb_out, d_image, npix * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(FIC_E_HIP, "fic_decode_rgb_run: %s", hipGetErrorString(e));
    }
    if (rc == FIC_OK && avg_error_io) *avg_error_io = avg;
    arena_give(ar);
    return rc;
}

int fic_decode_rgb_run(const uint8_t* run, int64_t len, int device, int32_t* argb_out, int64_t capacity_pixels,
                       int* w_out, int* h_out, float* avg_error_io, int* iterations)
{
    return fic_decode_rgb_run_zoom(run, len, 1, device, argb_out, capacity_pixels, w_out, h_out, avg_error_io, iterations);
}

// ---- fixed-B streams with an isometry column: tags 4 (grey) and 5 (colour), DESIGN.md 4.17 ------------------------------------
// Header {tag, w, h, 0, B, wK} -- the 0 where a .run holds its block size, so no older reader takes the stream --, then per
// range block in scanline order its quantised row and its isometry 0..7.
}  // extern "C"

namespace {
constexpr int kIsoHeaderInts = 6;
struct IsoStream {
    int tag, QW;             // ints of a quantised row: 3 grey {idx_local, qa, qb}, 5 colour {idx_local, q1, q2, q3, q4}
    const char *writer, *reader;
};
constexpr IsoStream kIsoGrey{4, 3, "fic_write_run_gray_iso", "fic_decode_gray_iso_run"},
                    kIsoRgb{5, 5, "fic_write_run_rgb_iso", "fic_decode_rgb_iso_run"};

int64_t write_iso_run(const IsoStream& S, const int32_t* qrows, const int32_t* iso, int n_ranges, int w, int h, int B, int wK,
                      uint8_t* out, int64_t capacity)
{
    if (!qrows || !iso || !out) return fail(FIC_E_ARGUMENT, "%s: null argument", S.writer);
    FicGeom g;
    const int rc = make_geometry(w, h, B, wK, 1, 1, &g);
    if (rc) return rc;
    if (n_ranges != g.Nr) return fail(FIC_E_ARGUMENT, "%s: %d rows, the %dx%d image has %d range blocks of side %d", S.writer, n_ranges, w, h, g.Nr, B);
    for (int j = 0; j < g.Nr; j++)
        if (iso[j] < 0 || iso[j] > 7) return fail(FIC_E_ARGUMENT, "%s: row %d: isometry %d outside 0..7", S.writer, j, iso[j]);
    const int per = S.QW + 1;
    const int64_t need = 4 * (kIsoHeaderInts + per * (int64_t)g.Nr);
    if (capacity < need) return fail(FIC_E_CAPACITY, "%s: need %lld bytes, have %lld", S.writer, (long long)need, (long long)capacity);
    const int32_t hdr[kIsoHeaderInts] = {S.tag, w, h, 0, B, wK};
    for (int i = 0; i < kIsoHeaderInts; i++) put_be32(out + 4 * i, hdr[i]);
    uint8_t* p = out + 4 * kIsoHeaderInts;
    for (int j = 0; j < g.Nr; j++) {
        for (int k = 0; k < S.QW; k++, p += 4) put_be32(p, qrows[(size_t)S.QW * j + k]);
        put_be32(p, iso[j]);
        p += 4;
    }
    return need;
}

// Reader + decoder: the stream checked on the host, rows and isometries uploaded, then the loop of the stream's twin
// (fic_decode_gray_run_zoom / fic_decode_rgb_run_zoom) with the isometry column handed to the paint kernel.
template <typename Px>
int decode_iso_run(const IsoStream& S, const uint8_t* run, int64_t len, int zoom, int device, Px* out, int64_t capacity, int* w_out,
                   int* h_out, float* avg_error_io, int* iterations)
{
    constexpr bool kRgb = sizeof(Px) == 4;
    if (!run || len < 4 * kIsoHeaderInts) return fail(FIC_E_ARGUMENT, "%s: stream shorter than the 24-byte header", S.reader);
    int32_t hd[kIsoHeaderInts];
    for (int i = 0; i < kIsoHeaderInts; i++) hd[i] = get_be32(run + 4 * i);
    if (hd[0] != S.tag || hd[3] != 0)
        return fail(FIC_E_ARGUMENT, "%s: header starts {%d, .., .., %d}, this stream has {%d, w, h, 0}", S.reader, hd[0], hd[3], S.tag);
    const int w0 = hd[1], h0 = hd[2], B = hd[4], wK = hd[5];
    FicGeom g0, g;
    int rc = make_geometry(w0, h0, B, wK, 1, 1, &g0);
    if (rc) return rc;
    const int per = S.QW + 1;
    const int64_t need = 4 * (kIsoHeaderInts + per * (int64_t)g0.Nr);
    if (len != need)
        return fail(FIC_E_ARGUMENT, "%s: %lld bytes, %d range blocks need exactly %lld", S.reader, (long long)len, g0.Nr, (long long)need);
    std::vector<int32_t> q((size_t)g0.Nr * S.QW), iso((size_t)g0.Nr);
    const uint8_t* p = run + 4 * kIsoHeaderInts;
    for (int j = 0; j < g0.Nr; j++) {
        for (int k = 0; k < S.QW; k++, p += 4) q[(size_t)S.QW * j + k] = get_be32(p);
        iso[j] = get_be32(p);
        p += 4;
        const int idx = q[(size_t)S.QW * j];
        if (idx < 0 || idx >= wK * wK || iso[j] < 0 || iso[j] > 7)
            return fail(FIC_E_ARGUMENT, "%s: row %d: idx_local %d outside the %dx%d window or isometry %d outside 0..7", S.reader, j, idx, wK, wK, iso[j]);
    }
    rc = make_decode_geometry(w0, h0, B, wK, 1, 1, zoom, &g);
    if (rc) return rc;
    const int w = g.W, h = g.H;
    if (w_out) *w_out = w;
    if (h_out) *h_out = h;
    const size_t npix = (size_t)w * h;
    if (!out || capacity < (int64_t)npix) return fail(FIC_E_CAPACITY, "%s: output needs %zu pixels", S.reader, npix);
    rc = check_device(device);
    if (rc) return rc;
    const size_t o_scaled = 0, o_image = o_scaled + align256((size_t)g.Ws * g.Hs * sizeof(Px)), o_q = o_image + align256(npix * sizeof(Px)),
                 o_iso = o_q + align256(q.size() * 4), o_state = o_iso + align256(iso.size() * 4),
                 o_sq = o_state + align256(sizeof(FicDecodeState)), total = o_sq + align256(fic_decode_sq_words(1, npix) * 4);
    Arena ar;
    rc = arena_take(device, total, &ar);
    if (rc) return rc;
    Px* d_scaled = (Px*)(ar.base + o_scaled);
    Px* d_image = (Px*)(ar.base + o_image);
    int32_t* d_q = (int32_t*)(ar.base + o_q);
    int32_t* d_iso = (int32_t*)(ar.base + o_iso);
    FicDecodeState* d_state = (FicDecodeState*)(ar.base + o_state);
    uint32_t* d_sq = (uint32_t*)(ar.base + o_sq);
    hipError_t e = hipMemcpy(d_q, q.data(), q.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_iso, iso.data(), iso.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) rc = fail(FIC_E_HIP, "%s: %s", S.reader, hipGetErrorString(e));
    float avg = avg_error_io ? *avg_error_io : 0.0f;
    if (rc == FIC_OK)
        rc = decode_loop(kRgb ? kDecodeRgb : kDecodeGrey, 1, npix, d_image, d_state, &avg, &avg, iterations, nullptr, nullptr, [&](int counter) {
            if constexpr (kRgb) return fic_launch_decode_iteration_rgb(d_scaled, d_image, d_q, d_state, d_sq, counter, g, nullptr, d_iso);
            else return fic_launch_decode_iteration(d_scaled, d_image, d_q, d_iso, d_state, d_sq, counter, g, nullptr);
        });
    if (rc == FIC_OK) {
        e = hipMemcpy(out, d_image, npix * sizeof(Px), hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(FIC_E_HIP, "%s: %s", S.reader, hipGetErrorString(e));
    }
    if (rc == FIC_OK && avg_error_io) *avg_error_io = avg;
    arena_give(ar);
    return rc;
}
}  // namespace

extern "C" {

int64_t fic_write_run_gray_iso(const int32_t* qrows, const int32_t* iso, int n_ranges, int w, int h, int B, int wK, uint8_t* out,
                               int64_t capacity)
{
    return write_iso_run(kIsoGrey, qrows, iso, n_ranges, w, h, B, wK, out, capacity);
}

int64_t fic_write_run_rgb_iso(const int32_t* qrows5, const int32_t* iso, int n_ranges, int w, int h, int B, int wK, uint8_t* out,
                              int64_t capacity)
{
    return write_iso_run(kIsoRgb, qrows5, iso, n_ranges, w, h, B, wK, out, capacity);
}

int fic_decode_gray_iso_run(const uint8_t* run, int64_t len, int zoom, int device, uint8_t* gray_out, int64_t capacity, int* w_out,
                            int* h_out, float* avg_error_io, int* iterations)
{
    return decode_iso_run<uint8_t>(kIsoGrey, run, len, zoom, device, gray_out, capacity, w_out, h_out, avg_error_io, iterations);
}

int fic_decode_rgb_iso_run(const uint8_t* run, int64_t len, int zoom, int device, int32_t* argb_out, int64_t capacity_pixels, int* w_out,
                           int* h_out, float* avg_error_io, int* iterations)
{
    return decode_iso_run<int32_t>(kIsoRgb, run, len, zoom, device, argb_out, capacity_pixels, w_out, h_out, avg_error_io, iterations);
}

}  // extern "C"
