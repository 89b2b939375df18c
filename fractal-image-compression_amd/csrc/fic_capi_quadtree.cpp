// fic_capi_quadtree.cpp -- C ABI, quadtree (variable block size) codec, grey and joint RGB: encode every level with the
// one-shot machinery, collage SSE + split + compaction on the device (fic_quadtree.hip), the tag-2 (grey), tag-3 (colour) and
// tag-6 (colour with an isometry column) stream writers / readers, and the decoders of leaves of mixed size.  Host-side
// orchestration only.  Semantics: DESIGN.md sections 4.13 (grey), 4.14 (colour) and 4.17 (colour with the 8 isometries).
#include "fic_internal.h"

using namespace ficd;

namespace {

constexpr int kQtMaxLevels = 3;   // 16 -> 8 -> 4
constexpr int kQtHeaderInts = 8;  // {2, w, h, B_max, B_min, wK, n_iso, n_leaves}; colour: {3 or 6, w, h, 0, B_max, B_min, wK, n_leaves}

// The levels B_max, B_max / 2, ..., B_min and their geometries (wK = 0: full search at every level, wK_B = Dw_B).
struct QtLevels {
    int nl = 0;
    FicGeom g[kQtMaxLevels];
};

int qt_levels(int w, int h, int B_max, int B_min, int wK, int n_iso, QtLevels* L)
{
    if (!((B_max == 8 || B_max == 16) && (B_min == 4 || B_min == 8) && B_min < B_max))
        return fail(FIC_E_ARGUMENT, "quadtree levels B_max=%d B_min=%d: need B_max in {8, 16}, B_min in {4, 8}, B_min < B_max", B_max, B_min);
    if (n_iso != 1 && n_iso != 8) return fail(FIC_E_ARGUMENT, "n_iso=%d: only 1 (reference) or 8 (extension)", n_iso);
    if (w <= 0 || h <= 0 || (w % B_max) || (h % B_max))
        return fail(FIC_E_GEOMETRY, "image %dx%d is not a positive multiple of B_max=%d", w, h, B_max);
    if (wK < 0) return fail(FIC_E_WINDOW, "widthKernel wK=%d: 0 (full search) or a window side", wK);
    if (wK == 0 && w != h) return fail(FIC_E_WINDOW, "wK = 0 (full search at every level) needs a square image, got %dx%d", w, h);
    L->nl = 0;
    for (int B = B_max; B >= B_min; B /= 2) {
        FicGeom g;
        int rc = make_geometry(w, h, B, 1, n_iso, 1, &g);
        if (rc == FIC_OK) rc = make_geometry(w, h, B, wK ? wK : g.Dw, n_iso, 1, &g);
        if (rc) return rc;
        L->g[L->nl++] = g;
    }
    return FIC_OK;
}

// window_to_global (fic_devfn.h; FC:128-150 with getDomainBlockIndex FC:516-545 and generateKernel FC:84-100) on the host,
// for the reader, which resolves every leaf's domain block once instead of on every iteration.
int host_window_to_global(const FicGeom& g, int j, int wloc)
{
    if (g.full) return wloc;
    int xr = j % g.Rw, yr = j / g.Rw, i = 0;
    if (yr == 0) yr = 1;
    if (xr == 0) xr = 1;
    if (yr == g.Rh - 1) yr = yr - 1;
    if (xr == g.Rw - 1) xr = xr - 1;
    if (xr > 1) i = (yr == 0) ? xr : (xr * 2) - 2 + (yr + yr - 1) * g.Dw;
    else if (xr == 1) i = (yr == 0) ? xr : xr + (yr + yr - 1) * g.Dw;
    int dy = i / g.Dw - g.wK / 2, dx = i % g.Dw - g.wK / 2;
    if (dx < 0) dx = 0;
    if (dy < 0) dy = 0;
    if (dx + g.wK >= g.Dw) dx = g.Dw - g.wK;
    if (dy + g.wK >= g.Dh) dy = g.Dh - g.wK;
    return dx + wloc % g.wK + (dy + wloc / g.wK) * g.Dw;
}

// Walks the leaves in stream order -- top-level blocks in scanline order, children TL, TR, BL, BR depth first -- with
// side(i) the side of leaf i, calling emit(i, x, y, level).  False when the sizes do not tile the image exactly with n leaves.
template <typename S, typename E>
bool qt_tile(const QtLevels& L, int n, S side, E emit)
{
    const int B_max = L.g[0].B;
    int i = 0;
    std::function<bool(int, int, int)> visit = [&](int x, int y, int l) -> bool {
        if (i >= n) return false;
        const int B = B_max >> l, b = side(i);
        if (b == B) {
            if (!emit(i, x, y, l)) return false;
            i++;
            return true;
        }
        if (b >= B || l + 1 >= L.nl) return false;
        const int hb = B / 2;
        return visit(x, y, l + 1) && visit(x + hb, y, l + 1) && visit(x, y + hb, l + 1) && visit(x + hb, y + hb, l + 1);
    };
    for (int y = 0; y < L.g[0].H; y += B_max)
        for (int x = 0; x < L.g[0].W; x += B_max)
            if (!visit(x, y, 0)) return false;
    return i == n;
}

// ---- the host side of a pixel format (QtGrey / QtRgb / QtRgbIso, fic_launch.h) --------------------------------------------
// The one-shot contexts an encode runs its levels through, their device buffers, the stream layout and the public names.
struct QtHeader {
    int w, h, B_max, B_min, wK, n_iso, n;
};
template <typename Px>
struct QtViews {
    const Px *image, *scaled;         // the input [H][W] and the 2:1 copy [Hs][Ws] the rows refer to
    const int32_t *qrows, *iso;
};

struct QtGreyHost : QtGrey {
    using Dev = QtGrey;               // the tag of the launchers
    using Ctx = fic_ctx;
    static constexpr const char *kKind = "quadtree", *kWriter = "fic_write_run_quadtree", *kReader = "fic_decode_quadtree_run";
    static constexpr const DecodeKind& kDecode = kDecodeGrey;
    static Ctx* take(int device, const FicGeom& g)
    {
        Ctx* c = cache_take(device, g.W, g.H, g.B, g.wK, g.n_iso);
        return c ? c : fic_ctx_create(device, g.W, g.H, g.B, g.wK, g.n_iso, 1);
    }
    static int encode(Ctx* c, const uint8_t* gray, const int32_t* argb)   // exactly the one-shot encode of this level
    {
        const int rc = gray ? fic_ctx_set_gray_host(c, gray) : fic_ctx_set_argb_host(c, argb);
        return rc ? rc : fic_ctx_encode(c, 0, -1, nullptr);
    }
    static void give(Ctx* c, bool ok) { ok ? cache_give(c) : fic_ctx_destroy(c); }
    // every level reads the top context's scaled copy, made here: the original, 2:1 scaled (FC:970-1007)
    static int prepare(Ctx* top) { return fic_launch_scale(top->b.gray, top->b.scaled, top->g, nullptr); }
    static QtViews<Px> views(const Ctx* c, const Ctx* top) { return {c->b.gray, top->b.scaled, c->o.qrows, c->g.n_iso > 1 ? c->o.iso : nullptr}; }
    static int scale(const Px* image, Px* scaled, const FicGeom& g) { return fic_launch_scale(image, scaled, g, nullptr); }
    static int run_ints(int n_iso) { return n_iso == 8 ? 5 : 4; }   // stream row {B, idx_local, qa, qb[, iso]}
    static void pack(const QtHeader& H, int32_t* hd)
    {
        const int32_t v[kQtHeaderInts] = {2, H.w, H.h, H.B_max, H.B_min, H.wK, H.n_iso, H.n};
        memcpy(hd, v, sizeof(v));
    }
    static int unpack(const int32_t* hd, QtHeader* H)
    {
        if (hd[0] != 2) return fail(FIC_E_ARGUMENT, "%s: tag %d, a quadtree stream has tag 2", kReader, hd[0]);
        *H = QtHeader{hd[1], hd[2], hd[3], hd[4], hd[5], hd[6], hd[7]};
        return FIC_OK;
    }
    static int levels_refused(int rc) { return rc; }
    static bool row_ok(const int32_t*) { return true; }              // the writer takes the iso column as it is
    // the leaf's row from the stream ints behind {B, idx_local}: {qa, qb[, iso]} -> q = {qa, qb, iso, 0}; returns the isometry
    static int fill(Leaf& e, const uint8_t* r, int n_iso)
    {
        e.q[0] = get_be32(r);
        e.q[1] = get_be32(r + 4);
        e.q[2] = n_iso == 8 ? get_be32(r + 8) : 0;
        return e.q[2];
    }
};

struct QtRgbHost : QtRgb {
    using Dev = QtRgb;
    using Ctx = fic_rgb_ctx;
    static constexpr const char *kKind = "colour quadtree", *kWriter = "fic_write_run_rgb_quadtree", *kReader = "fic_decode_rgb_quadtree_run";
    static constexpr const DecodeKind& kDecode = kDecodeRgb;
    static Ctx* take(int device, const FicGeom& g)
    {
        Ctx* c = rgb_cache_take(device, g.W, g.H, g.B, g.wK);
        return c ? c : fic_rgb_ctx_create(device, g.W, g.H, g.B, g.wK, 1);
    }
    static int encode(Ctx* c, const uint8_t*, const int32_t* argb)        // exactly the one-shot RGB encode of this level
    {
        const int rc = fic_rgb_ctx_set_argb_host(c, argb);
        return rc ? rc : fic_rgb_ctx_encode(c, 0, nullptr);
    }
    static void give(Ctx* c, bool ok) { ok ? rgb_cache_give(c) : fic_rgb_ctx_destroy(c); }
    static int prepare(Ctx*) { return 0; }
    static QtViews<Px> views(const Ctx* c, const Ctx*)   // every level reads its own scaleImageRGB copy, made by its encode
    {
        QtViews<Px> v{};
        rgb_ctx_views(c, &v.image, &v.scaled, &v.qrows);
        return v;
    }
    static int scale(const Px* image, Px* scaled, const FicGeom& g) { return fic_launch_scale_rgb(image, scaled, g, nullptr); }
    static int run_ints(int) { return 6; }                           // stream row {B, idx_local, q1, q2, q3, q4}
    static void pack(const QtHeader& H, int32_t* hd)
    {
        const int32_t v[kQtHeaderInts] = {3, H.w, H.h, 0, H.B_max, H.B_min, H.wK, H.n};   // 0 where the fixed-B .run holds B (FC:234-238)
        memcpy(hd, v, sizeof(v));
    }
    static int unpack(const int32_t* hd, QtHeader* H)
    {
        if (hd[0] != 3 || hd[3] != 0)
            return fail(FIC_E_ARGUMENT, "%s: header starts {%d, .., .., %d}, a colour quadtree stream has {3, w, h, 0}", kReader, hd[0], hd[3]);
        *H = QtHeader{hd[1], hd[2], hd[4], hd[5], hd[6], 1, hd[7]};
        return FIC_OK;
    }
    static int levels_refused(int) { return fail(FIC_E_ARGUMENT, "%s: %s", kReader, g_err.c_str()); }
    static bool row_ok(const int32_t*) { return true; }
    static int fill(Leaf& e, const uint8_t* r, int)                  // {q1, q2, q3, q4}, no isometry
    {
        for (int k = 0; k < 4; k++) e.q[k] = get_be32(r + 4 * k);
        return 0;
    }
};

// Colour with an isometry column: the joint-RGB contexts of n_iso = 1 or 8, tag 6.  The stream always holds
// the column (zeros for an n_iso = 1 codebook) and its reader takes every isometry 0..7.
struct QtRgbIsoHost : QtRgbIso {
    using Dev = QtRgbIso;
    using Ctx = fic_rgb_ctx;
    static constexpr const char *kKind = "colour quadtree (isometries)", *kWriter = "fic_write_run_rgb_quadtree_iso",
                                *kReader = "fic_decode_rgb_quadtree_iso_run";
    static constexpr const DecodeKind& kDecode = kDecodeRgb;
    static Ctx* take(int device, const FicGeom& g)
    {
        Ctx* c = rgb_cache_take(device, g.W, g.H, g.B, g.wK, g.n_iso);
        return c ? c : fic_rgb_ctx_create_iso(device, g.W, g.H, g.B, g.wK, g.n_iso, 1);
    }
    static int encode(Ctx* c, const uint8_t* gray, const int32_t* argb) { return QtRgbHost::encode(c, gray, argb); }   // = fic_encode_rgb_iso_argb's
    static void give(Ctx* c, bool ok) { QtRgbHost::give(c, ok); }
    static int prepare(Ctx*) { return 0; }
    static QtViews<Px> views(const Ctx* c, const Ctx*)
    {
        QtViews<Px> v{};
        rgb_ctx_views(c, &v.image, &v.scaled, &v.qrows, &v.iso);
        return v;
    }
    static int scale(const Px* image, Px* scaled, const FicGeom& g) { return fic_launch_scale_rgb(image, scaled, g, nullptr); }
    static int run_ints(int) { return 7; }                           // stream row {B, idx_local, q1, q2, q3, q4, iso}
    static void pack(const QtHeader& H, int32_t* hd)
    {
        const int32_t v[kQtHeaderInts] = {6, H.w, H.h, 0, H.B_max, H.B_min, H.wK, H.n};
        memcpy(hd, v, sizeof(v));
    }
    static int unpack(const int32_t* hd, QtHeader* H)
    {
        if (hd[0] != 6 || hd[3] != 0)
            return fail(FIC_E_ARGUMENT, "%s: header starts {%d, .., .., %d}, a colour quadtree stream with isometries has {6, w, h, 0}",
                        kReader, hd[0], hd[3]);
        *H = QtHeader{hd[1], hd[2], hd[4], hd[5], hd[6], 8, hd[7]};
        return FIC_OK;
    }
    static int levels_refused(int rc) { return rc; }                 // bad levels FIC_E_ARGUMENT, else the geometry's / window's own code
    static bool row_ok(const int32_t* leaf) { return leaf[8] >= 0 && leaf[8] <= 7; }
    static int fill(Leaf& e, const uint8_t* r, int)                  // {q1, q2, q3, q4, iso}
    {
        for (int k = 0; k < 4; k++) e.q[k] = get_be32(r + 4 * k);
        return e.k = get_be32(r + 16);
    }
};

// The encode behind fic_encode_*_quadtree_* and the SSE test hooks: every level through the one-shot contexts, then the
// per-level SSE, the split and the compaction on the device.  leaves / sse_out may be NULL.
template <typename Fmt>
int qt_encode(const uint8_t* gray, const int32_t* argb, int w, int h, int B_max, int B_min, int wK, int n_iso, float threshold,
              int device, int32_t* leaves, int64_t capacity, int* n_leaves, uint32_t* sse_out, int64_t sse_capacity)
{
    if (!gray && !argb) return fail(FIC_E_ARGUMENT, "%s encode: null image", Fmt::kKind);
    if (threshold != threshold) return fail(FIC_E_ARGUMENT, "%s encode: threshold is NaN", Fmt::kKind);
    QtLevels L;
    int rc = qt_levels(w, h, B_max, B_min, wK, n_iso, &L);
    if (rc) return rc;
    size_t sse_total = 0;
    for (int l = 0; l < L.nl; l++) sse_total += (size_t)L.g[l].Nr;
    if (sse_out && sse_capacity < (int64_t)sse_total)
        return fail(FIC_E_CAPACITY, "%s SSE: need %zu values, have %lld", Fmt::kKind, sse_total, (long long)sse_capacity);
    rc = check_device(device);
    if (rc) return rc;

    typename Fmt::Ctx* c[kQtMaxLevels] = {nullptr, nullptr, nullptr};
    char* scratch = nullptr;
    for (int l = 0; l < L.nl && rc == FIC_OK; l++) {
        c[l] = Fmt::take(device, L.g[l]);
        if (!c[l]) { rc = g_err_code ? g_err_code : FIC_E_HIP; break; }
        rc = Fmt::encode(c[l], gray, argb);
    }
    // scratch: SSE per level, counts / offsets per top-level block, the leaf table (room for every block of B_min)
    const FicGeom& top = L.g[0];
    const size_t max_leaves = (size_t)L.g[L.nl - 1].Nr;
    size_t o_sse[kQtMaxLevels], off = 0;
    for (int l = 0; l < L.nl; l++) { o_sse[l] = off; off += align256((size_t)L.g[l].Nr * 4); }
    const size_t o_cnt = off, o_offs = o_cnt + align256((size_t)top.Nr * 4), o_leaves = o_offs + align256(((size_t)top.Nr + 1) * 4),
                 total = o_leaves + align256(max_leaves * Fmt::kLeafInts * 4);
    if (rc == FIC_OK) rc = dev_alloc(&scratch, total);
    if (rc == FIC_OK && Fmt::prepare(c[0])) rc = fail(FIC_E_HIP, "k_scale launch failed");
    const uint32_t* sse[kQtMaxLevels];
    const int32_t* qrows[kQtMaxLevels];
    const int32_t* iso[kQtMaxLevels];
    int Rw[kQtMaxLevels];
    for (int l = 0; l < L.nl && rc == FIC_OK; l++) {
        const auto v = Fmt::views(c[l], c[0]);
        sse[l] = (const uint32_t*)(scratch + o_sse[l]);
        qrows[l] = v.qrows;
        iso[l] = v.iso;
        Rw[l] = L.g[l].Rw;
        if (fic_launch_leaf_sse<typename Fmt::Dev>(v.image, v.scaled, v.qrows, v.iso, (uint32_t*)(scratch + o_sse[l]), L.g[l], nullptr))
            rc = fail(FIC_E_HIP, "k_leaf_sse launch failed");
    }
    int* d_offs = (int*)(scratch + o_offs);
    if (rc == FIC_OK && fic_launch_qt_compact<typename Fmt::Dev>(sse, qrows, iso, Rw, L.nl, top.B, top.Rw, top.Nr, threshold,
                                                                 (int*)(scratch + o_cnt), d_offs, (int32_t*)(scratch + o_leaves), nullptr))
        rc = fail(FIC_E_HIP, "%s compaction launch failed", Fmt::kKind);
    int n = 0;
    if (rc == FIC_OK) {
        hipError_t e = hipMemcpy(&n, d_offs + top.Nr, sizeof(int), hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(FIC_E_HIP, "%s encode: %s", Fmt::kKind, hipGetErrorString(e));
    }
    if (rc == FIC_OK && n_leaves) *n_leaves = n;
    if (rc == FIC_OK && leaves) {
        if (capacity < n) rc = fail(FIC_E_CAPACITY, "%s encode: %d leaves, room for %lld", Fmt::kKind, n, (long long)capacity);
        else {
            hipError_t e = hipMemcpy(leaves, scratch + o_leaves, (size_t)n * Fmt::kLeafInts * 4, hipMemcpyDeviceToHost);
            if (e != hipSuccess) rc = fail(FIC_E_HIP, "%s encode: %s", Fmt::kKind, hipGetErrorString(e));
        }
    }
    for (int l = 0, o = 0; rc == FIC_OK && sse_out && l < L.nl; o += L.g[l].Nr, l++) {
        hipError_t e = hipMemcpy(sse_out + o, scratch + o_sse[l], (size_t)L.g[l].Nr * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(FIC_E_HIP, "%s SSE: %s", Fmt::kKind, hipGetErrorString(e));
    }
    ErrKeep keep;
    if (scratch) (void)hipFree(scratch);
    for (int l = 0; l < L.nl; l++)
        if (c[l]) Fmt::give(c[l], rc == FIC_OK);
    return rc;
}

// The stream writer: the header, then per leaf its row without the position, which follows from the order.
template <typename Fmt>
int64_t qt_write_run(const int32_t* leaves, int n_leaves, int w, int h, int B_max, int B_min, int wK, int n_iso, uint8_t* out,
                     int64_t capacity)
{
    if (!leaves || !out || n_leaves < 0) return fail(FIC_E_ARGUMENT, "%s: bad argument", Fmt::kWriter);
    QtLevels L;
    int rc = qt_levels(w, h, B_max, B_min, wK, n_iso, &L);
    if (rc) return rc;
    constexpr size_t LW = Fmt::kLeafInts;
    const bool tiles = qt_tile(L, n_leaves, [&](int i) { return leaves[LW * i + 2]; }, [&](int i, int x, int y, int) {
        return leaves[LW * i + 0] == x && leaves[LW * i + 1] == y;
    });
    if (!tiles) return fail(FIC_E_ARGUMENT, "%s: the leaves do not tile the %dx%d image in quadtree order", Fmt::kWriter, w, h);
    for (int i = 0; i < n_leaves; i++)
        if (!Fmt::row_ok(leaves + LW * i)) return fail(FIC_E_ARGUMENT, "%s: leaf %d: isometry outside 0..7", Fmt::kWriter, i);
    const int per = Fmt::run_ints(n_iso);
    const int64_t need = 4 * (kQtHeaderInts + per * (int64_t)n_leaves);
    if (capacity < need) return fail(FIC_E_CAPACITY, "%s: need %lld bytes, have %lld", Fmt::kWriter, (long long)need, (long long)capacity);
    int32_t hdr[kQtHeaderInts];
    Fmt::pack(QtHeader{w, h, B_max, B_min, wK, n_iso, n_leaves}, hdr);
    for (int i = 0; i < kQtHeaderInts; i++) put_be32(out + 4 * i, hdr[i]);
    uint8_t* p = out + 4 * kQtHeaderInts;
    for (int i = 0; i < n_leaves; i++)
        for (int k = 0; k < per; k++, p += 4) put_be32(p, leaves[LW * i + 2 + k]);
    return need;
}

// The stream reader and decoder: the leaves of every level resolved once on the host, then the decoder's loop with one paint
// per level and iteration.  zoom: every leaf {x, y, B} is painted as {zoom x, zoom y, zoom B} on the level's geometry times
// zoom (make_decode_geometry; the same block counts, so idx_local keeps its meaning), in the same stream order.
template <typename Fmt>
int qt_decode_run(const uint8_t* run, int64_t len, int zoom, int device, typename Fmt::Px* out, int64_t capacity_pixels, int* w_out, int* h_out,
                  float* avg_error_io, int* iterations)
{
    using Px = typename Fmt::Px;
    if (!run || len < 4 * kQtHeaderInts) return fail(FIC_E_ARGUMENT, "%s: stream shorter than the 32-byte header", Fmt::kReader);
    int32_t hd[kQtHeaderInts];
    for (int i = 0; i < kQtHeaderInts; i++) hd[i] = get_be32(run + 4 * i);
    QtHeader H;
    int rc = Fmt::unpack(hd, &H);
    if (rc) return rc;
    const int n = H.n;
    QtLevels L, Z;                                     // the stream's levels and the same at `zoom`, where the paint runs
    rc = qt_levels(H.w, H.h, H.B_max, H.B_min, H.wK, H.n_iso, &L);
    if (rc) return Fmt::levels_refused(rc);
    Z.nl = L.nl;
    for (int l = 0; l < L.nl; l++) {
        rc = make_decode_geometry(H.w, H.h, L.g[l].B, L.g[l].wK, H.n_iso, 1, zoom, &Z.g[l]);
        if (rc) return rc;
    }
    const int w = Z.g[0].W, h = Z.g[0].H;
    if (n < 1 || n > L.g[L.nl - 1].Nr) return fail(FIC_E_ARGUMENT, "%s: %d leaves", Fmt::kReader, n);
    const int per = Fmt::run_ints(H.n_iso);
    const int64_t need = 4 * (kQtHeaderInts + per * (int64_t)n);
    if (len != need)
        return fail(FIC_E_ARGUMENT, "%s: %lld bytes, %d leaves need exactly %lld", Fmt::kReader, (long long)len, n, (long long)need);
    const uint8_t* rows = run + 4 * kQtHeaderInts;
    using Leaf = typename Fmt::Leaf;
    std::vector<Leaf> lv[kQtMaxLevels];
    int sqoff = 0;
    const bool ok = qt_tile(L, n, [&](int i) { return get_be32(rows + 4 * per * (size_t)i); }, [&](int i, int x, int y, int l) {
        const FicGeom& g = L.g[l];
        const uint8_t* r = rows + 4 * per * (size_t)i;
        const int idx = get_be32(r + 4);
        Leaf e{};
        e.x = zoom * x; e.y = zoom * y; e.sqoff = sqoff;
        const int iso = Fmt::fill(e, r + 8, H.n_iso);
        if (idx < 0 || idx >= g.wK * g.wK || iso < 0 || iso >= H.n_iso) return false;
        e.gi = host_window_to_global(g, (y / g.B) * g.Rw + x / g.B, idx);
        if (e.gi < 0 || e.gi >= g.Nd) return false;
        lv[l].push_back(e);
        sqoff += Z.g[l].n;
        return true;
    });
    if (!ok)
        return fail(FIC_E_ARGUMENT, "%s: the leaf sizes do not tile the %dx%d image with levels %d..%d, or a leaf's domain index%s is "
                                    "out of range", Fmt::kReader, H.w, H.h, H.B_max, H.B_min, Fmt::kIso ? " / isometry" : "");
    if (w_out) *w_out = w;
    if (h_out) *h_out = h;
    const size_t npix = (size_t)w * h;
    if (!out || capacity_pixels < (int64_t)npix) return fail(FIC_E_CAPACITY, "%s: output needs %zu pixels", Fmt::kReader, npix);
    rc = check_device(device);
    if (rc) return rc;
    const FicGeom& g0 = Z.g[0];
    size_t o_lv[kQtMaxLevels];
    const size_t o_scaled = 0, o_image = o_scaled + align256((size_t)g0.Ws * g0.Hs * sizeof(Px));
    size_t off = o_image + align256(npix * sizeof(Px));
    for (int l = 0; l < L.nl; l++) { o_lv[l] = off; off += align256((lv[l].size() + 1) * sizeof(Leaf)); }
    const size_t o_state = off, o_sq = o_state + align256(sizeof(FicDecodeState)), total = o_sq + align256(fic_decode_sq_words(1, npix) * 4);
    Arena ar;
    rc = arena_take(device, total, &ar);
    if (rc) return rc;
    for (int l = 0; l < L.nl && rc == FIC_OK; l++) {
        if (lv[l].empty()) continue;
        hipError_t e = hipMemcpy(ar.base + o_lv[l], lv[l].data(), lv[l].size() * sizeof(Leaf), hipMemcpyHostToDevice);
        if (e != hipSuccess) rc = fail(FIC_E_HIP, "%s: %s", Fmt::kReader, hipGetErrorString(e));
    }
    Px* d_scaled = (Px*)(ar.base + o_scaled);
    Px* d_image = (Px*)(ar.base + o_image);
    FicDecodeState* d_state = (FicDecodeState*)(ar.base + o_state);
    uint32_t* d_sq = (uint32_t*)(ar.base + o_sq);
    float avg = avg_error_io ? *avg_error_io : 0.0f;
    // one iteration: scale the current image (FC:382, FC:459), paint the leaves level by level from that copy, loop control
    if (rc == FIC_OK)
        rc = decode_loop(Fmt::kDecode, 1, npix, d_image, d_state, &avg, &avg, iterations, nullptr, nullptr, [&](int counter) {
            if (Fmt::scale(d_image, d_scaled, g0)) return -1;
            for (int l = 0; l < L.nl; l++)
                if (fic_launch_decode_paint_leaves<typename Fmt::Dev>(d_scaled, d_image, (const Leaf*)(ar.base + o_lv[l]),
                                                                      (int)lv[l].size(), d_state, d_sq, counter, Z.g[l], nullptr))
                    return -1;
            return fic_launch_decode_step(d_state, d_sq, counter, (int)npix, 1, nullptr);
        });
    if (rc == FIC_OK) {
        hipError_t e = hipMemcpy(out, d_image, npix * sizeof(Px), hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(FIC_E_HIP, "%s: %s", Fmt::kReader, hipGetErrorString(e));
    }
    if (rc == FIC_OK && avg_error_io) *avg_error_io = avg;
    arena_give(ar);
    return rc;
}

}  // namespace

extern "C" {

int fic_encode_gray_quadtree_u8(const uint8_t* gray, int w, int h, int B_max, int B_min, int wK, int n_iso, float threshold,
                                int device, int32_t* leaves, int64_t capacity, int* n_leaves)
{
    if (!gray || !leaves || !n_leaves) return fail(FIC_E_ARGUMENT, "fic_encode_gray_quadtree_u8: null argument");
    return qt_encode<QtGreyHost>(gray, nullptr, w, h, B_max, B_min, wK, n_iso, threshold, device, leaves, capacity, n_leaves, nullptr, 0);
}

int fic_encode_gray_quadtree_argb(const int32_t* argb, int w, int h, int B_max, int B_min, int wK, int n_iso, float threshold,
                                  int device, int32_t* leaves, int64_t capacity, int* n_leaves)
{
    if (!argb || !leaves || !n_leaves) return fail(FIC_E_ARGUMENT, "fic_encode_gray_quadtree_argb: null argument");
    return qt_encode<QtGreyHost>(nullptr, argb, w, h, B_max, B_min, wK, n_iso, threshold, device, leaves, capacity, n_leaves, nullptr, 0);
}

int fic_debug_quadtree_sse(const uint8_t* gray, int w, int h, int B_max, int B_min, int wK, int n_iso, int device, uint32_t* sse,
                           int64_t capacity)
{
    if (!gray || !sse) return fail(FIC_E_ARGUMENT, "fic_debug_quadtree_sse: null argument");
    return qt_encode<QtGreyHost>(gray, nullptr, w, h, B_max, B_min, wK, n_iso, __builtin_inff(), device, nullptr, 0, nullptr, sse, capacity);
}

int64_t fic_write_run_quadtree(const int32_t* leaves, int n_leaves, int w, int h, int B_max, int B_min, int wK, int n_iso,
                               uint8_t* out, int64_t capacity)
{
    return qt_write_run<QtGreyHost>(leaves, n_leaves, w, h, B_max, B_min, wK, n_iso, out, capacity);
}

int fic_decode_quadtree_run_zoom(const uint8_t* run, int64_t len, int zoom, int device, uint8_t* gray_out, int64_t capacity, int* w_out,
                                 int* h_out, float* avg_error_io, int* iterations)
{
    return qt_decode_run<QtGreyHost>(run, len, zoom, device, gray_out, capacity, w_out, h_out, avg_error_io, iterations);
}

int fic_decode_quadtree_run(const uint8_t* run, int64_t len, int device, uint8_t* gray_out, int64_t capacity, int* w_out,
                            int* h_out, float* avg_error_io, int* iterations)
{
    return fic_decode_quadtree_run_zoom(run, len, 1, device, gray_out, capacity, w_out, h_out, avg_error_io, iterations);
}

int fic_encode_rgb_quadtree_argb(const int32_t* argb, int w, int h, int B_max, int B_min, int wK, float threshold, int device,
                                 int32_t* leaves, int64_t capacity, int* n_leaves)
{
    if (!argb || !leaves || !n_leaves) return fail(FIC_E_ARGUMENT, "fic_encode_rgb_quadtree_argb: null argument");
    return qt_encode<QtRgbHost>(nullptr, argb, w, h, B_max, B_min, wK, 1, threshold, device, leaves, capacity, n_leaves, nullptr, 0);
}

int fic_debug_rgb_quadtree_sse(const int32_t* argb, int w, int h, int B_max, int B_min, int wK, int device, uint32_t* sse,
                               int64_t capacity)
{
    if (!argb || !sse) return fail(FIC_E_ARGUMENT, "fic_debug_rgb_quadtree_sse: null argument");
    return qt_encode<QtRgbHost>(nullptr, argb, w, h, B_max, B_min, wK, 1, __builtin_inff(), device, nullptr, 0, nullptr, sse, capacity);
}

int64_t fic_write_run_rgb_quadtree(const int32_t* leaves, int n_leaves, int w, int h, int B_max, int B_min, int wK, uint8_t* out,
                                   int64_t capacity)
{
    return qt_write_run<QtRgbHost>(leaves, n_leaves, w, h, B_max, B_min, wK, 1, out, capacity);
}

int fic_decode_rgb_quadtree_run_zoom(const uint8_t* run, int64_t len, int zoom, int device, int32_t* argb_out, int64_t capacity_pixels,
                                     int* w_out, int* h_out, float* avg_error_io, int* iterations)
{
    return qt_decode_run<QtRgbHost>(run, len, zoom, device, argb_out, capacity_pixels, w_out, h_out, avg_error_io, iterations);
}

int fic_decode_rgb_quadtree_run(const uint8_t* run, int64_t len, int device, int32_t* argb_out, int64_t capacity_pixels, int* w_out,
                                int* h_out, float* avg_error_io, int* iterations)
{
    return fic_decode_rgb_quadtree_run_zoom(run, len, 1, device, argb_out, capacity_pixels, w_out, h_out, avg_error_io, iterations);
}

// ---- colour with the 8 isometries ------------------------------------------------------------------------
int fic_encode_rgb_quadtree_iso_argb(const int32_t* argb, int w, int h, int B_max, int B_min, int wK, int n_iso, float threshold,
                                     int device, int32_t* leaves, int64_t capacity, int* n_leaves)
{
    if (!argb || !leaves || !n_leaves) return fail(FIC_E_ARGUMENT, "fic_encode_rgb_quadtree_iso_argb: null argument");
    return qt_encode<QtRgbIsoHost>(nullptr, argb, w, h, B_max, B_min, wK, n_iso, threshold, device, leaves, capacity, n_leaves, nullptr, 0);
}

int fic_debug_rgb_quadtree_iso_sse(const int32_t* argb, int w, int h, int B_max, int B_min, int wK, int n_iso, int device,
                                   uint32_t* sse, int64_t capacity)
{
    if (!argb || !sse) return fail(FIC_E_ARGUMENT, "fic_debug_rgb_quadtree_iso_sse: null argument");
    return qt_encode<QtRgbIsoHost>(nullptr, argb, w, h, B_max, B_min, wK, n_iso, __builtin_inff(), device, nullptr, 0, nullptr, sse, capacity);
}

int64_t fic_write_run_rgb_quadtree_iso(const int32_t* leaves, int n_leaves, int w, int h, int B_max, int B_min, int wK, uint8_t* out,
                                       int64_t capacity)
{
    return qt_write_run<QtRgbIsoHost>(leaves, n_leaves, w, h, B_max, B_min, wK, 8, out, capacity);
}

int fic_decode_rgb_quadtree_iso_run(const uint8_t* run, int64_t len, int zoom, int device, int32_t* argb_out, int64_t capacity_pixels,
                                    int* w_out, int* h_out, float* avg_error_io, int* iterations)
{
    return qt_decode_run<QtRgbIsoHost>(run, len, zoom, device, argb_out, capacity_pixels, w_out, h_out, avg_error_io, iterations);
}

}  // extern "C"
