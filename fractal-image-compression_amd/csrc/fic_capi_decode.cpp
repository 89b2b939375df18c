// fic_capi_decode.cpp -- C ABI, decoder entries: FractalCompression.decode on .run streams (FC:547-553 -> decodeGreyScale
// FC:356-421, decodeRGB FC:430-508), the same with an isometry column (tags 4 and 5), and the decode of a context's own
// codebook.  Here too: the decode job every decoder of the library runs through (DecodeJob, fic_internal.h) with its arenas
// and the loop control.  The streams' bytes are parsed in fic_stream.cpp.  Host-side orchestration only.
#include "fic_internal.h"

using namespace ficd;

// ---- decoder (decodeGreyScale FC:356-421) ------------------------------------------------------
namespace {
// Device arenas of the decode jobs (struct Arena, fic_internal.h), kept between calls (the GUI decodes after every
// encode, CTL:178-179): one allocation per (device, size class) instead of four allocations and frees per call.
// fic_release_cache() frees them.
std::mutex g_arena_mu;
std::vector<Arena> g_arenas;
constexpr size_t kArenaSlots = 4;

int arena_take(int device, size_t bytes, Arena* out)
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
    return mem_alloc(kMemDevice, (void**)&out->base, bytes);
}
// an arena is its own (pointer, bytes) record: it goes back to the counted pair directly
void arena_free(const Arena& a)
{
    (void)hipSetDevice(a.device);
    mem_free(kMemDevice, a.base, a.bytes);
}
void arena_give(const Arena& a)
{
    Arena evict;
    {
        std::lock_guard<std::mutex> lk(g_arena_mu);
        g_arenas.push_back(a);
        if (g_arenas.size() <= kArenaSlots) return;
        evict = g_arenas.front();
        g_arenas.erase(g_arenas.begin());
    }
    arena_free(evict);
}

}  // namespace

void ficd::release_decoder_arenas()
{
    std::vector<Arena> drop;
    {
        std::lock_guard<std::mutex> lk(g_arena_mu);
        drop.swap(g_arenas);
    }
    for (const Arena& a : drop) arena_free(a);
}

static thread_local int g_last_sum_fallbacks = 0;

// Runs the reconstruction loop on the device.  The first 8 iterations are enqueued in one go, later ones in pairs, and the
// per-plane loop state is read back after each group (a converging decode takes 6-9 iterations): one host sync per
// group, none per iteration; iterations enqueued behind the last one exit at once.  `iteration(counter)` enqueues one
// iteration (scale, paint, loop control) on s; d_image [planes][npix] pixels of kind.px_bytes is filled with kind.px_start here.
//   d_state [planes]: scratch of the caller; st: the planes' final loop state (avg_out, iters, seq_sums), valid on FIC_OK
static int decode_loop(const DecodeKind& kind, int planes, size_t npix, void* d_image, FicDecodeState* d_state, const float* avg_in,
                       std::vector<FicDecodeState>& st, hipStream_t s, const std::function<int(int)>& iteration)
{
    const size_t P = (size_t)planes;
    st.resize(P);
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
    }
    return FIC_OK;
}

ficd::DecodeJob::~DecodeJob()
{
    if (arena.base) arena_give(arena);
}

void ficd::DecodeJob::borrow(const DecodeKind& k, const FicGeom& geom, hipStream_t s, void* d_scaled, void* d_image, FicDecodeState* d_state,
                       uint32_t* d_sq)
{
    kind = &k; g = geom; stream = s;
    scaled = d_scaled; image = d_image; state = d_state; sq = d_sq;
}

// The one layout of a decoder's workspace: scaled copy, image, the uploaded spans, loop state, sqbuf, each region starting on
// a multiple of 256 bytes behind the one before it.
int ficd::DecodeJob::open(const char* who, int device, const DecodeKind& k, const FicGeom& geom, hipStream_t s,
                    std::initializer_list<const std::vector<int32_t>*> upload)
{
    const size_t P = (size_t)geom.planes, npix = (size_t)geom.W * geom.H;
    std::vector<size_t> bytes{P * geom.Ws * geom.Hs * k.px_bytes, P * npix * k.px_bytes};
    for (const std::vector<int32_t>* v : upload) bytes.push_back(v->size() * sizeof(int32_t));
    bytes.push_back(P * sizeof(FicDecodeState));
    bytes.push_back(fic_decode_sq_words(P, npix) * sizeof(uint32_t));
    std::vector<size_t> at(bytes.size());
    size_t total = 0;
    for (size_t i = 0; i < bytes.size(); i++) { at[i] = total; total += align256(bytes[i]); }
    const int rc = arena_take(device, total, &arena);
    if (rc) return rc;
    const size_t n = upload.size();
    borrow(k, geom, s, arena.base + at[0], arena.base + at[1], (FicDecodeState*)(arena.base + at[2 + n]), (uint32_t*)(arena.base + at[3 + n]));
    size_t i = 2;
    for (const std::vector<int32_t>* v : upload) {
        if (!v->empty()) {
            const hipError_t e = hipMemcpy(arena.base + at[i], v->data(), bytes[i], hipMemcpyHostToDevice);
            if (e != hipSuccess) return fail(FIC_E_HIP, "%s: %s", who, hipGetErrorString(e));
        }
        spans.push_back((const int32_t*)(arena.base + at[i++]));
    }
    return FIC_OK;
}

int ficd::DecodeJob::run(const char* who, const float* avg_in, float* avg_out, int* iters_out, int* seq_out, void* host_out,
                   const std::function<int(int)>& iteration)
{
    const size_t P = (size_t)g.planes, npix = (size_t)g.W * g.H;
    std::vector<FicDecodeState> st;
    const int rc = decode_loop(*kind, g.planes, npix, image, state, avg_in, st, stream, iteration);
    if (rc) return rc;
    const hipError_t e = hipMemcpy(host_out, image, P * npix * kind->px_bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(FIC_E_HIP, "%s: %s", who, hipGetErrorString(e));
    for (size_t p = 0; p < P; p++) {
        if (avg_out) avg_out[p] = st[p].avg_out;
        if (iters_out) iters_out[p] = st[p].iters;
        if (seq_out) seq_out[p] = st[p].seq_sums;
    }
    return FIC_OK;
}

namespace {

// one iteration of a fixed-block decode of either pixel format: rows [planes][N_r][QW], iso [planes][N_r] or NULL (identity)
std::function<int(int)> fixed_iteration(const DecodeJob& J, const int32_t* rows, const int32_t* iso)
{
    return [&J, rows, iso](int counter) {
        return J.kind->px_bytes == 1
            ? fic_launch_decode_iteration((uint8_t*)J.scaled, (uint8_t*)J.image, rows, iso, J.state, J.sq, counter, J.g, J.stream)
            : fic_launch_decode_iteration_rgb((int32_t*)J.scaled, (int32_t*)J.image, rows, J.state, J.sq, counter, J.g, J.stream, iso);
    };
}

// Reader + decoder of the four fixed-block tags: the stream parsed (and, tags 4 and 5, checked) on the host, rows and
// isometries uploaded, then the loop.
int decode_fixed_run(const FixedFormat& F, const uint8_t* run, int64_t len, int zoom, int device, void* out, int64_t capacity, int* w_out,
                     int* h_out, float* avg_error_io, int* iterations, int* seq_sums)
{
    FixedStream S;
    int rc = parse_fixed(F, run, len, zoom, &S);
    if (S.sized && w_out) *w_out = S.gz.W;             // also of a .run stream whose body is short (parse_fixed)
    if (S.sized && h_out) *h_out = S.gz.H;
    if (rc) return rc;
    const DecodeKind& kind = F.QW == 3 ? kDecodeGrey : kDecodeRgb;
    const long long npix = (long long)S.gz.W * S.gz.H;
    if (!out || capacity < npix) return fail(FIC_E_CAPACITY, "%s: output needs %lld %s", F.reader, npix, kind.px_bytes == 1 ? "bytes" : "ints");
    rc = check_device(device);
    if (rc) return rc;
    DecodeJob J;
    rc = F.iso ? J.open(F.reader, device, kind, S.gz, nullptr, {&S.rows, &S.iso}) : J.open(F.reader, device, kind, S.gz, nullptr, {&S.rows});
    if (rc) return rc;
    return J.run(F.reader, avg_error_io, avg_error_io, iterations, seq_sums, out, fixed_iteration(J, J.spans[0], F.iso ? J.spans[1] : nullptr));
}

}  // namespace

extern "C" {

int fic_ctx_decode_zoom_host(fic_ctx* c, int zoom, uint8_t* gray_out, float* avg_error_out, int* iterations_out)
{
    if (!c || !gray_out) return fail(FIC_E_ARGUMENT, "fic_ctx_decode_host: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->encoded_any) return fail(FIC_E_STATE, "fic_ctx_decode_host: nothing encoded yet");
    DecodeJob J;
    if (zoom != 1) {
        // the context's own scratch holds the encoded size: a zoomed decode takes an arena of the zoomed size instead
        FicGeom g;
        int rc = make_decode_geometry(c->g.W, c->g.H, c->g.B, c->g.wK, c->g.n_iso, c->g.planes, zoom, &g);
        if (rc) return rc;
        HIP_TRY(hipSetDevice(c->device));
        rc = J.open("fic_ctx_decode_zoom_host", c->device, kDecodeGrey, g, c->last_stream);
        if (rc) return rc;
    } else {
        HIP_TRY(hipSetDevice(c->device));
        const FicGeom& g = c->g;
        const size_t P = (size_t)g.planes, npix = (size_t)g.W * g.H;
        if (int rc = c->mem.ensure(c->decoded, P * npix)) return rc;
        if (int rc = c->mem.ensure(c->dec_state, P)) return rc;
        if (int rc = c->mem.ensure(c->dec_sq, fic_decode_sq_words(P, npix))) return rc;
        J.borrow(kDecodeGrey, g, c->last_stream, c->b.scaled, c->decoded, c->dec_state, c->dec_sq);
    }
    HIP_TRY(hipStreamSynchronize(c->last_stream));
    return J.run("fic_ctx_decode_zoom_host", nullptr, avg_error_out, iterations_out, nullptr, gray_out,
                 fixed_iteration(J, c->o.qrows, c->g.n_iso > 1 ? c->o.iso : nullptr));
}

int fic_ctx_decode_host(fic_ctx* c, uint8_t* gray_out, float* avg_error_out, int* iterations_out)
{
    return fic_ctx_decode_zoom_host(c, 1, gray_out, avg_error_out, iterations_out);
}

int fic_decode_gray_run_zoom(const uint8_t* run, int64_t len, int zoom, int device, uint8_t* gray_out, int64_t capacity, int* w_out,
                             int* h_out, float* avg_error_io, int* iterations)
{
    return decode_fixed_run(kRunGrey, run, len, zoom, device, gray_out, capacity, w_out, h_out, avg_error_io, iterations, nullptr);
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
    DevMem scratch(device);
    uint32_t* d = nullptr;
    float* r = nullptr;
    uint32_t* maps = nullptr;
    rc = scratch.alloc(d, (size_t)count + 4);
    if (rc == FIC_OK) rc = scratch.alloc(r, 2);
    if (rc == FIC_OK) rc = scratch.alloc(maps, fic_float_sum_map_words((size_t)count) + 4);
    if (rc) return rc;
    hipError_t e = hipMemcpy(d, vals, (size_t)count * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(FIC_E_HIP, "fic_debug_float_sum: %s", hipGetErrorString(e));
    if (fic_launch_float_sum_probe(carry, d, count, maps, r, nullptr)) return fail(FIC_E_HIP, "k_float_sum_probe launch failed");
    float two[2] = {0.0f, 0.0f};
    e = hipMemcpy(two, r, 8, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(FIC_E_HIP, "fic_debug_float_sum: %s", hipGetErrorString(e));
    out[0] = two[0];
    g_last_sum_fallbacks = (int)two[1];
    return FIC_OK;
}

// Test hook: segments of the last fic_debug_float_sum on this thread that went through the sequential-order path.
int fic_debug_float_sum_fallbacks(void) { return g_last_sum_fallbacks; }

// Test hook: fic_decode_gray_run that also reports how many iterations needed the sequential (Java-order) float sum.
int fic_debug_decode_gray_run(const uint8_t* run, int64_t len, int device, uint8_t* gray_out, int64_t capacity,
                              float* avg_error_io, int* iterations, int* seq_sums)
{
    return decode_fixed_run(kRunGrey, run, len, 1, device, gray_out, capacity, nullptr, nullptr, avg_error_io, iterations, seq_sums);
}

// ---- decodeRGB (FC:430-508) -----------------------------------------------------------------------
int fic_decode_rgb_run_zoom(const uint8_t* run, int64_t len, int zoom, int device, int32_t* argb_out, int64_t capacity_pixels,
                            int* w_out, int* h_out, float* avg_error_io, int* iterations)
{
    return decode_fixed_run(kRunRgb, run, len, zoom, device, argb_out, capacity_pixels, w_out, h_out, avg_error_io, iterations, nullptr);
}

int fic_decode_rgb_run(const uint8_t* run, int64_t len, int device, int32_t* argb_out, int64_t capacity_pixels,
                       int* w_out, int* h_out, float* avg_error_io, int* iterations)
{
    return fic_decode_rgb_run_zoom(run, len, 1, device, argb_out, capacity_pixels, w_out, h_out, avg_error_io, iterations);
}

// ---- fixed-B streams with an isometry column: tags 4 (grey) and 5 (colour), DESIGN.md 4.17 ------------------------------------
int fic_decode_gray_iso_run(const uint8_t* run, int64_t len, int zoom, int device, uint8_t* gray_out, int64_t capacity, int* w_out,
                            int* h_out, float* avg_error_io, int* iterations)
{
    return decode_fixed_run(kIsoGrey, run, len, zoom, device, gray_out, capacity, w_out, h_out, avg_error_io, iterations, nullptr);
}

int fic_decode_rgb_iso_run(const uint8_t* run, int64_t len, int zoom, int device, int32_t* argb_out, int64_t capacity_pixels, int* w_out,
                           int* h_out, float* avg_error_io, int* iterations)
{
    return decode_fixed_run(kIsoRgb, run, len, zoom, device, argb_out, capacity_pixels, w_out, h_out, avg_error_io, iterations, nullptr);
}

}  // extern "C"
