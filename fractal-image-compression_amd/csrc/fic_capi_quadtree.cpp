// fic_capi_quadtree.cpp -- C ABI, quadtree (variable block size) codec, grey and joint RGB: encode every level with the
// one-shot machinery, collage SSE + split + compaction on the device (fic_quadtree.hip), the tag-2 (grey) and tag-3 (colour)
// stream writers / readers, and the decoders of leaves of mixed size.  Host-side orchestration only.  Semantics: DESIGN.md
// sections 4.13 (grey) and 4.14 (colour).
#include "fic_internal.h"

using namespace ficd;

namespace {

constexpr int kQtMaxLevels = 3;   // 16 -> 8 -> 4
constexpr int kQtHeaderInts = 8;  // {2, w, h, B_max, B_min, wK, n_iso, n_leaves}; colour: {3, w, h, 0, B_max, B_min, wK, n_leaves}
constexpr int kQtRgbLeafInts = 8; // colour leaf table row {x, y, B, idx_local, q1, q2, q3, q4}
constexpr int kQtRgbRunInts = 6;  // colour stream row {B, idx_local, q1, q2, q3, q4}

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

int check_device(int device)
{
    int ndev = fic_device_count();
    if (ndev <= 0 || device < 0 || device >= ndev) return fail(FIC_E_NO_DEVICE, "no HIP device %d (this library has no CPU path)", device);
    HIP_TRY(hipSetDevice(device));
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

void put_be32(uint8_t* p, int32_t v)
{
    uint32_t u = (uint32_t)v;
    p[0] = (uint8_t)(u >> 24); p[1] = (uint8_t)(u >> 16); p[2] = (uint8_t)(u >> 8); p[3] = (uint8_t)u;
}
int32_t get_be32(const uint8_t* p)
{
    return (int32_t)(((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3]);
}

// The encode behind fic_encode_gray_quadtree_* and the SSE test hook: every level through the one-shot contexts, then the
// per-level SSE, the split and the compaction on the device.  leaves / sse_out may be NULL.
int qt_encode(const uint8_t* gray, const int32_t* argb, int w, int h, int B_max, int B_min, int wK, int n_iso, float threshold,
              int device, int32_t* leaves, int64_t capacity, int* n_leaves, uint32_t* sse_out, int64_t sse_capacity)
{
    if (!gray && !argb) return fail(FIC_E_ARGUMENT, "quadtree encode: null image");
    if (threshold != threshold) return fail(FIC_E_ARGUMENT, "quadtree encode: threshold is NaN");
    QtLevels L;
    int rc = qt_levels(w, h, B_max, B_min, wK, n_iso, &L);
    if (rc) return rc;
    size_t sse_total = 0;
    for (int l = 0; l < L.nl; l++) sse_total += (size_t)L.g[l].Nr;
    if (sse_out && sse_capacity < (int64_t)sse_total)
        return fail(FIC_E_CAPACITY, "quadtree SSE: need %zu values, have %lld", sse_total, (long long)sse_capacity);
    rc = check_device(device);
    if (rc) return rc;

    fic_ctx* c[kQtMaxLevels] = {nullptr, nullptr, nullptr};
    char* scratch = nullptr;
    for (int l = 0; l < L.nl && rc == FIC_OK; l++) {
        const FicGeom& g = L.g[l];
        c[l] = cache_take(device, w, h, g.B, g.wK, n_iso);
        if (!c[l]) c[l] = fic_ctx_create(device, w, h, g.B, g.wK, n_iso, 1);
        if (!c[l]) { rc = g_err_code ? g_err_code : FIC_E_HIP; break; }
        rc = gray ? fic_ctx_set_gray_host(c[l], gray) : fic_ctx_set_argb_host(c[l], argb);
        if (rc == FIC_OK) rc = fic_ctx_encode(c[l], 0, -1, nullptr);   // exactly the one-shot encode of this level
    }
    // scratch: SSE per level, counts / offsets per top-level block, the leaf table (room for every block of B_min)
    const FicGeom& top = L.g[0];
    const size_t max_leaves = (size_t)L.g[L.nl - 1].Nr;
    size_t o_sse[kQtMaxLevels], off = 0;
    for (int l = 0; l < L.nl; l++) { o_sse[l] = off; off += align256((size_t)L.g[l].Nr * 4); }
    const size_t o_cnt = off, o_offs = o_cnt + align256((size_t)top.Nr * 4), o_leaves = o_offs + align256(((size_t)top.Nr + 1) * 4),
                 total = o_leaves + align256(max_leaves * 7 * 4);
    if (rc == FIC_OK) rc = dev_alloc(&scratch, total);
    if (rc == FIC_OK && fic_launch_scale(c[0]->b.gray, c[0]->b.scaled, top, nullptr))   // the original, 2:1 scaled (FC:970-1007)
        rc = fail(FIC_E_HIP, "k_scale launch failed");
    const uint32_t* sse[kQtMaxLevels];
    const int32_t* qrows[kQtMaxLevels];
    const int32_t* iso[kQtMaxLevels];
    int Rw[kQtMaxLevels];
    for (int l = 0; l < L.nl && rc == FIC_OK; l++) {
        sse[l] = (const uint32_t*)(scratch + o_sse[l]);
        qrows[l] = c[l]->o.qrows;
        iso[l] = n_iso > 1 ? c[l]->o.iso : nullptr;
        Rw[l] = L.g[l].Rw;
        if (fic_launch_leaf_sse(c[l]->b.gray, c[0]->b.scaled, qrows[l], iso[l], (uint32_t*)(scratch + o_sse[l]), L.g[l], nullptr))
            rc = fail(FIC_E_HIP, "k_leaf_sse launch failed");
    }
    int* d_offs = (int*)(scratch + o_offs);
    if (rc == FIC_OK && fic_launch_qt_compact(sse, qrows, iso, Rw, L.nl, top.B, top.Rw, top.Nr, threshold, (int*)(scratch + o_cnt),
                                              d_offs, (int32_t*)(scratch + o_leaves), nullptr))
        rc = fail(FIC_E_HIP, "quadtree compaction launch failed");
    int n = 0;
    if (rc == FIC_OK) {
        hipError_t e = hipMemcpy(&n, d_offs + top.Nr, sizeof(int), hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(FIC_E_HIP, "quadtree encode: %s", hipGetErrorString(e));
    }
    if (rc == FIC_OK && n_leaves) *n_leaves = n;
    if (rc == FIC_OK && leaves) {
        if (capacity < n) rc = fail(FIC_E_CAPACITY, "quadtree encode: %d leaves, room for %lld", n, (long long)capacity);
        else {
            hipError_t e = hipMemcpy(leaves, scratch + o_leaves, (size_t)n * 7 * 4, hipMemcpyDeviceToHost);
            if (e != hipSuccess) rc = fail(FIC_E_HIP, "quadtree encode: %s", hipGetErrorString(e));
        }
    }
    for (int l = 0, o = 0; rc == FIC_OK && sse_out && l < L.nl; o += L.g[l].Nr, l++) {
        hipError_t e = hipMemcpy(sse_out + o, scratch + o_sse[l], (size_t)L.g[l].Nr * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(FIC_E_HIP, "quadtree SSE: %s", hipGetErrorString(e));
    }
    ErrKeep keep;
    if (scratch) (void)hipFree(scratch);
    for (int l = 0; l < L.nl; l++) {
        if (!c[l]) continue;
        if (rc == FIC_OK) cache_give(c[l]);
        else fic_ctx_destroy(c[l]);
    }
    return rc;
}

// The colour twin of qt_encode behind fic_encode_rgb_quadtree_argb and its SSE hook: every level through the one-shot RGB
// contexts (fic_encode_rgb_argb's cache), then the per-level SSE over the three channels, the split and the compaction.
int qt_encode_rgb(const int32_t* argb, int w, int h, int B_max, int B_min, int wK, float threshold, int device, int32_t* leaves,
                  int64_t capacity, int* n_leaves, uint32_t* sse_out, int64_t sse_capacity)
{
    if (!argb) return fail(FIC_E_ARGUMENT, "colour quadtree encode: null image");
    if (threshold != threshold) return fail(FIC_E_ARGUMENT, "colour quadtree encode: threshold is NaN");
    QtLevels L;
    int rc = qt_levels(w, h, B_max, B_min, wK, 1, &L);
    if (rc) return rc;
    size_t sse_total = 0;
    for (int l = 0; l < L.nl; l++) sse_total += (size_t)L.g[l].Nr;
    if (sse_out && sse_capacity < (int64_t)sse_total)
        return fail(FIC_E_CAPACITY, "colour quadtree SSE: need %zu values, have %lld", sse_total, (long long)sse_capacity);
    rc = check_device(device);
    if (rc) return rc;

    fic_rgb_ctx* c[kQtMaxLevels] = {nullptr, nullptr, nullptr};
    char* scratch = nullptr;
    for (int l = 0; l < L.nl && rc == FIC_OK; l++) {
        const FicGeom& g = L.g[l];
        c[l] = rgb_cache_take(device, w, h, g.B, g.wK);
        if (!c[l]) c[l] = fic_rgb_ctx_create(device, w, h, g.B, g.wK, 1);
        if (!c[l]) { rc = g_err_code ? g_err_code : FIC_E_HIP; break; }
        rc = fic_rgb_ctx_set_argb_host(c[l], argb);
        if (rc == FIC_OK) rc = fic_rgb_ctx_encode(c[l], 0, nullptr);   // exactly the one-shot RGB encode of this level
    }
    const FicGeom& top = L.g[0];
    const size_t max_leaves = (size_t)L.g[L.nl - 1].Nr;
    size_t o_sse[kQtMaxLevels], off = 0;
    for (int l = 0; l < L.nl; l++) { o_sse[l] = off; off += align256((size_t)L.g[l].Nr * 4); }
    const size_t o_cnt = off, o_offs = o_cnt + align256((size_t)top.Nr * 4), o_leaves = o_offs + align256(((size_t)top.Nr + 1) * 4),
                 total = o_leaves + align256(max_leaves * kQtRgbLeafInts * 4);
    if (rc == FIC_OK) rc = dev_alloc(&scratch, total);
    const uint32_t* sse[kQtMaxLevels];
    const int32_t* qrows[kQtMaxLevels];
    const int32_t* no_iso[kQtMaxLevels] = {nullptr, nullptr, nullptr};
    int Rw[kQtMaxLevels];
    for (int l = 0; l < L.nl && rc == FIC_OK; l++) {
        const int32_t *d_argb, *d_scaled;   // the context's input and its scaleImageRGB copy, made by the encode
        rgb_ctx_views(c[l], &d_argb, &d_scaled, &qrows[l]);
        sse[l] = (const uint32_t*)(scratch + o_sse[l]);
        Rw[l] = L.g[l].Rw;
        if (fic_launch_leaf_sse_rgb(d_argb, d_scaled, qrows[l], (uint32_t*)(scratch + o_sse[l]), L.g[l], nullptr))
            rc = fail(FIC_E_HIP, "k_leaf_sse_rgb launch failed");
    }
    int* d_offs = (int*)(scratch + o_offs);
    if (rc == FIC_OK && fic_launch_qt_compact(sse, qrows, no_iso, Rw, L.nl, top.B, top.Rw, top.Nr, threshold, (int*)(scratch + o_cnt),
                                              d_offs, (int32_t*)(scratch + o_leaves), nullptr, 5))
        rc = fail(FIC_E_HIP, "colour quadtree compaction launch failed");
    int n = 0;
    if (rc == FIC_OK) {
        hipError_t e = hipMemcpy(&n, d_offs + top.Nr, sizeof(int), hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(FIC_E_HIP, "colour quadtree encode: %s", hipGetErrorString(e));
    }
    if (rc == FIC_OK && n_leaves) *n_leaves = n;
    if (rc == FIC_OK && leaves) {
        if (capacity < n) rc = fail(FIC_E_CAPACITY, "colour quadtree encode: %d leaves, room for %lld", n, (long long)capacity);
        else {
            hipError_t e = hipMemcpy(leaves, scratch + o_leaves, (size_t)n * kQtRgbLeafInts * 4, hipMemcpyDeviceToHost);
            if (e != hipSuccess) rc = fail(FIC_E_HIP, "colour quadtree encode: %s", hipGetErrorString(e));
        }
    }
    for (int l = 0, o = 0; rc == FIC_OK && sse_out && l < L.nl; o += L.g[l].Nr, l++) {
        hipError_t e = hipMemcpy(sse_out + o, scratch + o_sse[l], (size_t)L.g[l].Nr * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(FIC_E_HIP, "colour quadtree SSE: %s", hipGetErrorString(e));
    }
    ErrKeep keep;
    if (scratch) (void)hipFree(scratch);
    for (int l = 0; l < L.nl; l++) {
        if (!c[l]) continue;
        if (rc == FIC_OK) rgb_cache_give(c[l]);
        else fic_rgb_ctx_destroy(c[l]);
    }
    return rc;
}

}  // namespace

extern "C" {

int fic_encode_gray_quadtree_u8(const uint8_t* gray, int w, int h, int B_max, int B_min, int wK, int n_iso, float threshold,
                                int device, int32_t* leaves, int64_t capacity, int* n_leaves)
{
    if (!gray || !leaves || !n_leaves) return fail(FIC_E_ARGUMENT, "fic_encode_gray_quadtree_u8: null argument");
    return qt_encode(gray, nullptr, w, h, B_max, B_min, wK, n_iso, threshold, device, leaves, capacity, n_leaves, nullptr, 0);
}

int fic_encode_gray_quadtree_argb(const int32_t* argb, int w, int h, int B_max, int B_min, int wK, int n_iso, float threshold,
                                  int device, int32_t* leaves, int64_t capacity, int* n_leaves)
{
    if (!argb || !leaves || !n_leaves) return fail(FIC_E_ARGUMENT, "fic_encode_gray_quadtree_argb: null argument");
    return qt_encode(nullptr, argb, w, h, B_max, B_min, wK, n_iso, threshold, device, leaves, capacity, n_leaves, nullptr, 0);
}

int fic_debug_quadtree_sse(const uint8_t* gray, int w, int h, int B_max, int B_min, int wK, int n_iso, int device, uint32_t* sse,
                           int64_t capacity)
{
    if (!gray || !sse) return fail(FIC_E_ARGUMENT, "fic_debug_quadtree_sse: null argument");
    return qt_encode(gray, nullptr, w, h, B_max, B_min, wK, n_iso, __builtin_inff(), device, nullptr, 0, nullptr, sse, capacity);
}

int64_t fic_write_run_quadtree(const int32_t* leaves, int n_leaves, int w, int h, int B_max, int B_min, int wK, int n_iso,
                               uint8_t* out, int64_t capacity)
{
    if (!leaves || !out || n_leaves < 0) return fail(FIC_E_ARGUMENT, "fic_write_run_quadtree: bad argument");
    QtLevels L;
    int rc = qt_levels(w, h, B_max, B_min, wK, n_iso, &L);
    if (rc) return rc;
    const bool tiles = qt_tile(L, n_leaves, [&](int i) { return leaves[7 * (size_t)i + 2]; }, [&](int i, int x, int y, int) {
        return leaves[7 * (size_t)i + 0] == x && leaves[7 * (size_t)i + 1] == y;
    });
    if (!tiles) return fail(FIC_E_ARGUMENT, "fic_write_run_quadtree: the leaves do not tile the %dx%d image in quadtree order", w, h);
    const int per = n_iso == 8 ? 5 : 4;
    const int64_t need = 4 * (kQtHeaderInts + per * (int64_t)n_leaves);
    if (capacity < need) return fail(FIC_E_CAPACITY, "fic_write_run_quadtree: need %lld bytes, have %lld", (long long)need, (long long)capacity);
    const int32_t hdr[kQtHeaderInts] = {2, w, h, B_max, B_min, wK, n_iso, n_leaves};
    for (int i = 0; i < kQtHeaderInts; i++) put_be32(out + 4 * i, hdr[i]);
    uint8_t* p = out + 4 * kQtHeaderInts;
    for (int i = 0; i < n_leaves; i++) {
        const int32_t* r = leaves + 7 * (size_t)i;
        const int32_t row[5] = {r[2], r[3], r[4], r[5], r[6]};   // {B, idx_local, qa, qb[, iso]}: positions follow from the order
        for (int k = 0; k < per; k++, p += 4) put_be32(p, row[k]);
    }
    return need;
}

int fic_decode_quadtree_run(const uint8_t* run, int64_t len, int device, uint8_t* gray_out, int64_t capacity, int* w_out,
                            int* h_out, float* avg_error_io, int* iterations)
{
    if (!run || len < 4 * kQtHeaderInts) return fail(FIC_E_ARGUMENT, "fic_decode_quadtree_run: stream shorter than the 32-byte header");
    int32_t hd[kQtHeaderInts];
    for (int i = 0; i < kQtHeaderInts; i++) hd[i] = get_be32(run + 4 * i);
    if (hd[0] != 2) return fail(FIC_E_ARGUMENT, "fic_decode_quadtree_run: tag %d, a quadtree stream has tag 2", hd[0]);
    const int w = hd[1], h = hd[2], B_max = hd[3], B_min = hd[4], wK = hd[5], n_iso = hd[6], n = hd[7];
    QtLevels L;
    int rc = qt_levels(w, h, B_max, B_min, wK, n_iso, &L);
    if (rc) return rc;
    if (n < 1 || n > L.g[L.nl - 1].Nr) return fail(FIC_E_ARGUMENT, "fic_decode_quadtree_run: %d leaves", n);
    const int per = n_iso == 8 ? 5 : 4;
    const int64_t need = 4 * (kQtHeaderInts + per * (int64_t)n);
    if (len != need)
        return fail(FIC_E_ARGUMENT, "fic_decode_quadtree_run: %lld bytes, %d leaves need exactly %lld", (long long)len, n, (long long)need);
    const uint8_t* rows = run + 4 * kQtHeaderInts;
    std::vector<FicQtLeaf> lv[kQtMaxLevels];
    int sqoff = 0;
    const bool ok = qt_tile(L, n, [&](int i) { return get_be32(rows + 4 * per * (size_t)i); }, [&](int i, int x, int y, int l) {
        const FicGeom& g = L.g[l];
        const uint8_t* r = rows + 4 * per * (size_t)i;
        const int idx = get_be32(r + 4), k = per == 5 ? get_be32(r + 16) : 0;
        if (idx < 0 || idx >= g.wK * g.wK || k < 0 || k >= n_iso) return false;
        const int gi = host_window_to_global(g, (y / g.B) * g.Rw + x / g.B, idx);
        if (gi < 0 || gi >= g.Nd) return false;
        lv[l].push_back(FicQtLeaf{x, y, gi, sqoff, get_be32(r + 8), get_be32(r + 12), k, 0});
        sqoff += g.n;
        return true;
    });
    if (!ok)
        return fail(FIC_E_ARGUMENT, "fic_decode_quadtree_run: the leaf sizes do not tile the %dx%d image with levels %d..%d, or a leaf's "
                                    "domain index / isometry is out of range", w, h, B_max, B_min);
    if (w_out) *w_out = w;
    if (h_out) *h_out = h;
    const size_t npix = (size_t)w * h;
    if (!gray_out || capacity < (int64_t)npix) return fail(FIC_E_CAPACITY, "fic_decode_quadtree_run: output needs %zu bytes", npix);
    rc = check_device(device);
    if (rc) return rc;
    const FicGeom& g0 = L.g[0];
    size_t o_lv[kQtMaxLevels];
    const size_t o_scaled = 0, o_image = o_scaled + align256((size_t)g0.Ws * g0.Hs);
    size_t off = o_image + align256(npix);
    for (int l = 0; l < L.nl; l++) { o_lv[l] = off; off += align256((lv[l].size() + 1) * sizeof(FicQtLeaf)); }
    const size_t o_state = off, o_sq = o_state + align256(sizeof(FicDecodeState)), total = o_sq + align256(fic_decode_sq_words(1, npix) * 4);
    Arena ar;
    rc = arena_take(device, total, &ar);
    if (rc) return rc;
    for (int l = 0; l < L.nl && rc == FIC_OK; l++) {
        if (lv[l].empty()) continue;
        hipError_t e = hipMemcpy(ar.base + o_lv[l], lv[l].data(), lv[l].size() * sizeof(FicQtLeaf), hipMemcpyHostToDevice);
        if (e != hipSuccess) rc = fail(FIC_E_HIP, "fic_decode_quadtree_run: %s", hipGetErrorString(e));
    }
    uint8_t* d_scaled = (uint8_t*)(ar.base + o_scaled);
    uint8_t* d_image = (uint8_t*)(ar.base + o_image);
    FicDecodeState* d_state = (FicDecodeState*)(ar.base + o_state);
    uint32_t* d_sq = (uint32_t*)(ar.base + o_sq);
    float avg = avg_error_io ? *avg_error_io : 0.0f;
    // one iteration: scale the current image (FC:382), paint the leaves level by level from that copy, loop control
    if (rc == FIC_OK)
        rc = decode_loop(1, npix, d_image, d_state, &avg, &avg, iterations, nullptr, nullptr, [&](int counter) {
            if (fic_launch_scale(d_image, d_scaled, g0, nullptr)) return -1;
            for (int l = 0; l < L.nl; l++)
                if (fic_launch_decode_paint_leaves(d_scaled, d_image, (const FicQtLeaf*)(ar.base + o_lv[l]), (int)lv[l].size(), d_state,
                                                   d_sq, counter, L.g[l], nullptr))
                    return -1;
            return fic_launch_decode_step(d_state, d_sq, counter, (int)npix, 1, nullptr);
        });
    if (rc == FIC_OK) {
        hipError_t e = hipMemcpy(gray_out, d_image, npix, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(FIC_E_HIP, "fic_decode_quadtree_run: %s", hipGetErrorString(e));
    }
    if (rc == FIC_OK && avg_error_io) *avg_error_io = avg;
    arena_give(ar);
    return rc;
}

int fic_encode_rgb_quadtree_argb(const int32_t* argb, int w, int h, int B_max, int B_min, int wK, float threshold, int device,
                                 int32_t* leaves, int64_t capacity, int* n_leaves)
{
    if (!argb || !leaves || !n_leaves) return fail(FIC_E_ARGUMENT, "fic_encode_rgb_quadtree_argb: null argument");
    return qt_encode_rgb(argb, w, h, B_max, B_min, wK, threshold, device, leaves, capacity, n_leaves, nullptr, 0);
}

int fic_debug_rgb_quadtree_sse(const int32_t* argb, int w, int h, int B_max, int B_min, int wK, int device, uint32_t* sse,
                               int64_t capacity)
{
    if (!argb || !sse) return fail(FIC_E_ARGUMENT, "fic_debug_rgb_quadtree_sse: null argument");
    return qt_encode_rgb(argb, w, h, B_max, B_min, wK, __builtin_inff(), device, nullptr, 0, nullptr, sse, capacity);
}

int64_t fic_write_run_rgb_quadtree(const int32_t* leaves, int n_leaves, int w, int h, int B_max, int B_min, int wK, uint8_t* out,
                                   int64_t capacity)
{
    if (!leaves || !out || n_leaves < 0) return fail(FIC_E_ARGUMENT, "fic_write_run_rgb_quadtree: bad argument");
    QtLevels L;
    int rc = qt_levels(w, h, B_max, B_min, wK, 1, &L);
    if (rc) return rc;
    const int32_t* lv = leaves;
    const bool tiles = qt_tile(L, n_leaves, [&](int i) { return lv[kQtRgbLeafInts * (size_t)i + 2]; }, [&](int i, int x, int y, int) {
        return lv[kQtRgbLeafInts * (size_t)i + 0] == x && lv[kQtRgbLeafInts * (size_t)i + 1] == y;
    });
    if (!tiles) return fail(FIC_E_ARGUMENT, "fic_write_run_rgb_quadtree: the leaves do not tile the %dx%d image in quadtree order", w, h);
    const int64_t need = 4 * (kQtHeaderInts + kQtRgbRunInts * (int64_t)n_leaves);
    if (capacity < need)
        return fail(FIC_E_CAPACITY, "fic_write_run_rgb_quadtree: need %lld bytes, have %lld", (long long)need, (long long)capacity);
    const int32_t hdr[kQtHeaderInts] = {3, w, h, 0, B_max, B_min, wK, n_leaves};   // 0 where the fixed-B .run holds B (FC:234-238)
    for (int i = 0; i < kQtHeaderInts; i++) put_be32(out + 4 * i, hdr[i]);
    uint8_t* p = out + 4 * kQtHeaderInts;
    for (int i = 0; i < n_leaves; i++)    // {B, idx_local, q1, q2, q3, q4}: positions follow from the order
        for (int k = 2; k < kQtRgbLeafInts; k++, p += 4) put_be32(p, leaves[kQtRgbLeafInts * (size_t)i + k]);
    return need;
}

int fic_decode_rgb_quadtree_run(const uint8_t* run, int64_t len, int device, int32_t* argb_out, int64_t capacity_pixels, int* w_out,
                                int* h_out, float* avg_error_io, int* iterations)
{
    if (!run || len < 4 * kQtHeaderInts)
        return fail(FIC_E_ARGUMENT, "fic_decode_rgb_quadtree_run: stream shorter than the 32-byte header");
    int32_t hd[kQtHeaderInts];
    for (int i = 0; i < kQtHeaderInts; i++) hd[i] = get_be32(run + 4 * i);
    if (hd[0] != 3 || hd[3] != 0)
        return fail(FIC_E_ARGUMENT, "fic_decode_rgb_quadtree_run: header starts {%d, .., .., %d}, a colour quadtree stream has {3, w, h, 0}",
                    hd[0], hd[3]);
    const int w = hd[1], h = hd[2], B_max = hd[4], B_min = hd[5], wK = hd[6], n = hd[7];
    QtLevels L;
    if (qt_levels(w, h, B_max, B_min, wK, 1, &L))
        return fail(FIC_E_ARGUMENT, "fic_decode_rgb_quadtree_run: %s", g_err.c_str());
    if (n < 1 || n > L.g[L.nl - 1].Nr) return fail(FIC_E_ARGUMENT, "fic_decode_rgb_quadtree_run: %d leaves", n);
    const int64_t need = 4 * (kQtHeaderInts + kQtRgbRunInts * (int64_t)n);
    if (len != need)
        return fail(FIC_E_ARGUMENT, "fic_decode_rgb_quadtree_run: %lld bytes, %d leaves need exactly %lld", (long long)len, n,
                    (long long)need);
    const uint8_t* rows = run + 4 * kQtHeaderInts;
    constexpr size_t row_bytes = 4 * kQtRgbRunInts;
    std::vector<FicQtLeafRgb> lv[kQtMaxLevels];
    int sqoff = 0;
    const bool ok = qt_tile(L, n, [&](int i) { return get_be32(rows + row_bytes * (size_t)i); }, [&](int i, int x, int y, int l) {
        const FicGeom& g = L.g[l];
        const uint8_t* r = rows + row_bytes * (size_t)i;
        const int idx = get_be32(r + 4);
        if (idx < 0 || idx >= g.wK * g.wK) return false;
        const int gi = host_window_to_global(g, (y / g.B) * g.Rw + x / g.B, idx);
        if (gi < 0 || gi >= g.Nd) return false;
        lv[l].push_back(FicQtLeafRgb{x, y, gi, sqoff, get_be32(r + 8), get_be32(r + 12), get_be32(r + 16), get_be32(r + 20)});
        sqoff += g.n;
        return true;
    });
    if (!ok)
        return fail(FIC_E_ARGUMENT, "fic_decode_rgb_quadtree_run: the leaf sizes do not tile the %dx%d image with levels %d..%d, or a "
                                    "leaf's domain index is out of range", w, h, B_max, B_min);
    if (w_out) *w_out = w;
    if (h_out) *h_out = h;
    const size_t npix = (size_t)w * h;
    if (!argb_out || capacity_pixels < (int64_t)npix)
        return fail(FIC_E_CAPACITY, "fic_decode_rgb_quadtree_run: output needs %zu pixels", npix);
    int rc = check_device(device);
    if (rc) return rc;
    const FicGeom& g0 = L.g[0];
    size_t o_lv[kQtMaxLevels];
    const size_t o_scaled = 0, o_image = o_scaled + align256((size_t)g0.Ws * g0.Hs * 4);
    size_t off = o_image + align256(npix * 4);
    for (int l = 0; l < L.nl; l++) { o_lv[l] = off; off += align256((lv[l].size() + 1) * sizeof(FicQtLeafRgb)); }
    const size_t o_state = off, o_sq = o_state + align256(sizeof(FicDecodeState)), total = o_sq + align256(fic_decode_sq_words(1, npix) * 4);
    Arena ar;
    rc = arena_take(device, total, &ar);
    if (rc) return rc;
    for (int l = 0; l < L.nl && rc == FIC_OK; l++) {
        if (lv[l].empty()) continue;
        hipError_t e = hipMemcpy(ar.base + o_lv[l], lv[l].data(), lv[l].size() * sizeof(FicQtLeafRgb), hipMemcpyHostToDevice);
        if (e != hipSuccess) rc = fail(FIC_E_HIP, "fic_decode_rgb_quadtree_run: %s", hipGetErrorString(e));
    }
    int32_t* d_scaled = (int32_t*)(ar.base + o_scaled);
    int32_t* d_image = (int32_t*)(ar.base + o_image);
    FicDecodeState* d_state = (FicDecodeState*)(ar.base + o_state);
    uint32_t* d_sq = (uint32_t*)(ar.base + o_sq);
    float avg = avg_error_io ? *avg_error_io : 0.0f;
    // one iteration: scaleImageRGB of the current image (FC:459), paint the leaves level by level from that copy, loop control.
    // decode_loop fills the image with grey bytes; the colour start is generateGrayImage's 0xff808080 (FC:1142-1148).
    if (rc == FIC_OK)
        rc = decode_loop(1, npix, (uint8_t*)d_image, d_state, &avg, &avg, iterations, nullptr, nullptr, [&](int counter) {
            if (counter == 0 && hipMemsetD32Async((hipDeviceptr_t)d_image, (int)0xff808080u, npix, nullptr) != hipSuccess) return -1;
            if (fic_launch_scale_rgb(d_image, d_scaled, g0, nullptr)) return -1;
            for (int l = 0; l < L.nl; l++)
                if (fic_launch_decode_paint_leaves_rgb(d_scaled, d_image, (const FicQtLeafRgb*)(ar.base + o_lv[l]), (int)lv[l].size(),
                                                       d_state, d_sq, counter, L.g[l], nullptr))
                    return -1;
            return fic_launch_decode_step(d_state, d_sq, counter, (int)npix, 1, nullptr);
        });
    if (rc == FIC_OK) {
        hipError_t e = hipMemcpy(argb_out, d_image, npix * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(FIC_E_HIP, "fic_decode_rgb_quadtree_run: %s", hipGetErrorString(e));
    }
    if (rc == FIC_OK && avg_error_io) *avg_error_io = avg;
    arena_give(ar);
    return rc;
}

}  // extern "C"
