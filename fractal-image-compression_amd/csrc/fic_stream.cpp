// fic_stream.cpp -- the stream formats of fic_stream.h: the one writer and the one parser of the fixed-block tags (0, 1, 4, 5)
// and of the quadtree tags (2, 3, 6), the C ABI's writers, and the host code under them (error state, geometry).  The parsers
// are the only code of the library that reads bytes it did not write: everything here is plain C++, no HIP header and no HIP
// call, and tests/cpp/stream_parse_test.cpp runs it under the host compiler's sanitizers.
#include "fic_stream.h"

#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <functional>

namespace ficd {

thread_local std::string g_err;
thread_local int g_err_code = 0;

int fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    g_err_code = code;
    return code;
}

static int ilog2(int v)
{
    int l = 0;
    while ((1 << l) < v) l++;
    return l;
}

// Geometry as the reference derives it (FC:111-116, FC:1019-1022) + what it needs to not throw.  B_top: the largest side taken.
static int geometry_for(int w, int h, int B, int wK, int n_iso, int planes, int B_top, FicGeom* out)
{
    if (B != 4 && B != 8 && B != 16 && !(B_top >= B && (B == 32 || B == 64)))
        return fail(FIC_E_GEOMETRY, "blockgroesse B=%d unsupported (GUI values 4, 8, 16; B=2 divides by zero at FC:1022)", B);
    if (w <= 0 || h <= 0 || (w % 2) || (h % 2))
        return fail(FIC_E_GEOMETRY, "image %dx%d: width and height must be positive and even (scaleImage FC:970-1007 overruns otherwise)", w, h);
    if ((w % B) || (h % B))
        return fail(FIC_E_GEOMETRY, "image %dx%d is not a multiple of B=%d (ArrayIndexOutOfBounds in the reference)", w, h, B);
    if ((long long)w * h >= 0x7FFFFFFFll)              // before any product of block counts: a header may hold any two ints
        return fail(FIC_E_GEOMETRY, "image %dx%d too large for 32-bit candidate indices", w, h);
    FicGeom g;
    memset(&g, 0, sizeof(g));
    g.W = w; g.H = h; g.B = B; g.n = B * B; g.lgn = ilog2(B * B);
    g.Ws = w / 2; g.Hs = h / 2; g.abstand = B / 4;
    g.Rw = w / B; g.Rh = h / B; g.Nr = g.Rw * g.Rh;
    g.Dw = g.Rw * 2 - 3; g.Dh = g.Rh * 2 - 3;
    if (g.Dw < 1 || g.Dh < 1)
        return fail(FIC_E_GEOMETRY, "image %dx%d with B=%d has no domain blocks (Dw=%d Dh=%d)", w, h, B, g.Dw, g.Dh);
    g.Nd = g.Dw * g.Dh;
    if ((long long)g.Nd * 8 >= 0x7FFFFFFFll)
        return fail(FIC_E_GEOMETRY, "image %dx%d too large for 32-bit candidate indices", w, h);
    if (out == nullptr) return FIC_OK;
    if (wK < 1 || wK > g.Dw || wK > g.Dh)
        return fail(FIC_E_WINDOW, "widthKernel wK=%d outside 1..min(Dw=%d,Dh=%d) (negative index at FC:145)", wK, g.Dw, g.Dh);
    if (n_iso != 1 && n_iso != 8) return fail(FIC_E_ARGUMENT, "n_iso=%d: only 1 (reference) or 8 (extension)", n_iso);
    if (planes < 1) return fail(FIC_E_ARGUMENT, "planes=%d", planes);
    g.wK = wK; g.n_iso = n_iso; g.planes = planes;
    g.DW = g.n / 4;
    int NR = 1, NC = 1;
    fic_fast_variant(B, n_iso, &NR, &NC);
    g.NR = NR;
    int tsz = 64 * NR;
    g.tiles = (g.Nr + tsz - 1) / tsz;
    g.Nr_pad = g.tiles * tsz;
    g.Nd_pad = g.Nd + FIC_POOL_PAD;
    g.full = (wK == g.Dw && wK == g.Dh) ? 1 : 0;
    *out = g;
    return FIC_OK;
}

int make_geometry(int w, int h, int B, int wK, int n_iso, int planes, FicGeom* out) { return geometry_for(w, h, B, wK, n_iso, planes, 16, out); }

// The geometry (zoom * w, zoom * h, zoom * B, wK) a stream of the valid geometry (w, h, B, wK) decodes on at zoom 1, 2 or 4:
// the same block counts, so every row keeps its meaning.  The sides 32 and 64 exist for the decoders only.
int make_decode_geometry(int w, int h, int B, int wK, int n_iso, int planes, int zoom, FicGeom* out)
{
    if (zoom != 1 && zoom != 2 && zoom != 4) return fail(FIC_E_ARGUMENT, "zoom=%d: only 1, 2 or 4", zoom);
    if ((long long)w * zoom >= 0x7FFFFFFFll || (long long)h * zoom >= 0x7FFFFFFFll)
        return fail(FIC_E_GEOMETRY, "image %dx%d at zoom %d too large for 32-bit candidate indices", w, h, zoom);
    return geometry_for(w * zoom, h * zoom, B * zoom, wK, n_iso, planes, 64, out);
}

// ---- fixed block size: tags 0, 1, 4, 5 ------------------------------------------------------------------------------------------
// writeData (FC:234-256) and its twins with a column: the header, then per range block in scanline order its row[, isometry]
int64_t write_fixed(const FixedFormat& F, const int32_t* rows, const int32_t* iso, int n_ranges, int w, int h, int B, int wK,
                    uint8_t* out, int64_t capacity)
{
    if (!rows || !out || n_ranges < 0 || (F.iso && !iso)) return fail(FIC_E_ARGUMENT, "%s: bad argument", F.writer);
    if (F.host_checked) {
        FicGeom g;
        const int rc = make_geometry(w, h, B, wK, 1, 1, &g);
        if (rc) return rc;
        if (n_ranges != g.Nr) return fail(FIC_E_ARGUMENT, "%s: %d rows, the %dx%d image has %d range blocks of side %d", F.writer, n_ranges, w, h, g.Nr, B);
        for (int j = 0; j < g.Nr; j++)
            if (iso[j] < 0 || iso[j] > 7) return fail(FIC_E_ARGUMENT, "%s: row %d: isometry %d outside 0..7", F.writer, j, iso[j]);
    }
    const int64_t need = 4 * (F.header_ints + (F.QW + (F.iso ? 1 : 0)) * (int64_t)n_ranges);
    if (capacity < need) return fail(FIC_E_CAPACITY, "%s: need %lld bytes, have %lld", F.writer, (long long)need, (long long)capacity);
    const int32_t run_hdr[5] = {F.tag, w, h, B, wK}, iso_hdr[6] = {F.tag, w, h, 0, B, wK};     // FC:234-238
    uint8_t* p = out;
    for (int i = 0; i < F.header_ints; i++, p += 4) put_be32(p, F.header_ints == 5 ? run_hdr[i] : iso_hdr[i]);
    for (int j = 0; j < n_ranges; j++) {                                                      // FC:241-256
        for (int k = 0; k < F.QW; k++, p += 4) put_be32(p, rows[(size_t)F.QW * j + k]);
        if (F.iso) { put_be32(p, iso[j]); p += 4; }
    }
    return need;
}

// The header's geometry (w, h, B, wK) must be one the encoders take; the decode runs on it times `zoom`.  A .run reader sizes
// the image from the header before it looks at the body, as decodeGreyScale / decodeRGB do (FC:362-371): out->sized is set
// even when the body then turns out short.  A checked format reports no size before the whole stream has passed.
int parse_fixed(const FixedFormat& F, const uint8_t* run, int64_t len, int zoom, FixedStream* out)
{
    const int H = F.header_ints, per = F.QW + (F.iso ? 1 : 0);
    if (!run || len < 4 * H) return fail(FIC_E_ARGUMENT, "%s: stream shorter than the %d-byte header", F.reader, 4 * H);
    int32_t hd[6];
    for (int i = 0; i < H; i++) hd[i] = get_be32(run + 4 * i);
    if (H == 5 && F.tag == 0 && hd[0] != 0)
        return fail(FIC_E_NOT_GREY, "%s: isRGB = %d (FC:548-552 dispatches to decodeRGB)", F.reader, hd[0]);
    if (H == 5 && F.tag != 0 && hd[0] == 0) return fail(FIC_E_ARGUMENT, "%s: isRGB = 0 (FC:548-550 dispatches to decodeGreyScale)", F.reader);
    if (H == 6 && (hd[0] != F.tag || hd[3] != 0))
        return fail(FIC_E_ARGUMENT, "%s: header starts {%d, .., .., %d}, this stream has {%d, w, h, 0}", F.reader, hd[0], hd[3], F.tag);
    const int w = hd[1], h = hd[2], B = hd[H - 2], wK = hd[H - 1];
    int rc = make_geometry(w, h, B, wK, 1, 1, &out->g);
    if (rc == FIC_OK && !F.host_checked) {
        rc = make_decode_geometry(w, h, B, wK, 1, 1, zoom, &out->gz);
        out->sized = rc == FIC_OK;
    }
    if (rc) return rc;
    const int Nr = out->g.Nr;
    const int64_t need = 4 * (H + per * (int64_t)Nr);
    if (F.exact ? len != need : len < need)
        return F.exact ? fail(FIC_E_ARGUMENT, "%s: %lld bytes, %d range blocks need exactly %lld", F.reader, (long long)len, Nr, (long long)need)
                       : fail(FIC_E_ARGUMENT, "%s: %lld bytes, need %lld (EOFException in the reference)", F.reader, (long long)len, (long long)need);
    out->rows.resize((size_t)Nr * F.QW);
    out->iso.resize(F.iso ? (size_t)Nr : 0);
    const uint8_t* p = run + 4 * H;
    if (!F.iso && !F.host_checked)                                                            // FC:372-374, FC:446-450
        for (size_t i = 0; i < out->rows.size(); i++) out->rows[i] = get_be32(p + 4 * i);
    else
        for (int j = 0; j < Nr; j++, p += 4 * per) {                                          // every row checked as it is read
            int32_t* row = &out->rows[(size_t)F.QW * j];
            for (int k = 0; k < F.QW; k++) row[k] = get_be32(p + 4 * k);
            const int iso = F.iso ? (out->iso[j] = get_be32(p + 4 * F.QW)) : 0;
            if (F.host_checked && (row[0] < 0 || row[0] >= wK * wK || iso < 0 || iso > 7))
                return fail(FIC_E_ARGUMENT, "%s: row %d: idx_local %d outside the %dx%d window or isometry %d outside 0..7", F.reader, j, row[0], wK, wK, iso);
        }
    if (!F.host_checked) return FIC_OK;
    rc = make_decode_geometry(w, h, B, wK, 1, 1, zoom, &out->gz);
    out->sized = rc == FIC_OK;
    return rc;
}

// ---- quadtree: tags 2, 3, 6 -----------------------------------------------------------------------------------------------------
constexpr int kQtHeaderInts = 8;
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
static int host_window_to_global(const FicGeom& g, int j, int wloc)
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
static bool qt_tile(const QtLevels& L, int n, S side, E emit)
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

// ints of a stream row {B, row[, iso]}
static int qt_run_ints(const QtFormat& F, int n_iso) { return 1 + F.QW + ((F.iso || (F.tag == 2 && n_iso == 8)) ? 1 : 0); }

// The header, then per leaf its row without the position, which follows from the order.
int64_t write_quadtree(const QtFormat& F, const int32_t* leaves, int n_leaves, int w, int h, int B_max, int B_min, int wK, int n_iso,
                       uint8_t* out, int64_t capacity)
{
    if (!leaves || !out || n_leaves < 0) return fail(FIC_E_ARGUMENT, "%s: bad argument", F.writer);
    QtLevels L;
    int rc = qt_levels(w, h, B_max, B_min, wK, n_iso, &L);
    if (rc) return rc;
    const size_t LW = (size_t)F.leaf_ints;
    const bool tiles = qt_tile(L, n_leaves, [&](int i) { return leaves[LW * i + 2]; }, [&](int i, int x, int y, int) {
        return leaves[LW * i + 0] == x && leaves[LW * i + 1] == y;
    });
    if (!tiles) return fail(FIC_E_ARGUMENT, "%s: the leaves do not tile the %dx%d image in quadtree order", F.writer, w, h);
    for (int i = 0; F.iso && i < n_leaves; i++)        // tag 2 takes its column as it is
        if (leaves[LW * i + LW - 1] < 0 || leaves[LW * i + LW - 1] > 7) return fail(FIC_E_ARGUMENT, "%s: leaf %d: isometry outside 0..7", F.writer, i);
    const int per = qt_run_ints(F, n_iso);
    const int64_t need = 4 * (kQtHeaderInts + per * (int64_t)n_leaves);
    if (capacity < need) return fail(FIC_E_CAPACITY, "%s: need %lld bytes, have %lld", F.writer, (long long)need, (long long)capacity);
    const int32_t grey[kQtHeaderInts] = {2, w, h, B_max, B_min, wK, n_iso, n_leaves},
                  colour[kQtHeaderInts] = {F.tag, w, h, 0, B_max, B_min, wK, n_leaves};   // 0 where the fixed-B .run holds B (FC:234-238)
    uint8_t* p = out;
    for (int i = 0; i < kQtHeaderInts; i++, p += 4) put_be32(p, F.tag == 2 ? grey[i] : colour[i]);
    for (int i = 0; i < n_leaves; i++)
        for (int k = 0; k < per; k++, p += 4) put_be32(p, leaves[LW * i + 2 + k]);
    return need;
}

// The leaves of every level resolved once on the host.  zoom: every leaf {x, y, B} is painted as {zoom x, zoom y, zoom B} on the
// level's geometry times zoom (make_decode_geometry; the same block counts, so idx_local keeps its meaning), in the same order.
int parse_quadtree(const QtFormat& F, const uint8_t* run, int64_t len, int zoom, QtStream* out)
{
    if (!run || len < 4 * kQtHeaderInts) return fail(FIC_E_ARGUMENT, "%s: stream shorter than the 32-byte header", F.reader);
    int32_t hd[kQtHeaderInts];
    for (int i = 0; i < kQtHeaderInts; i++) hd[i] = get_be32(run + 4 * i);
    const bool grey = F.tag == 2;
    if (grey && hd[0] != 2) return fail(FIC_E_ARGUMENT, "%s: tag %d, a quadtree stream has tag 2", F.reader, hd[0]);
    if (!grey && (hd[0] != F.tag || hd[3] != 0))
        return fail(FIC_E_ARGUMENT, "%s: header starts {%d, .., .., %d}, a %s stream has {%d, w, h, 0}", F.reader, hd[0], hd[3], F.kind, F.tag);
    const int w = hd[1], h = hd[2], B_max = hd[grey ? 3 : 4], B_min = hd[grey ? 4 : 5], wK = hd[grey ? 5 : 6], n = hd[7];
    const int n_iso = grey ? hd[6] : (F.iso ? 8 : 1);
    QtLevels &L = out->L, &Z = out->Z;
    int rc = qt_levels(w, h, B_max, B_min, wK, n_iso, &L);
    // the tag-3 reader reports whatever its levels are refused for as a bad argument; tags 2 and 6: bad levels
    // FIC_E_ARGUMENT, else the geometry's / window's own code
    if (rc) return F.tag == 3 ? fail(FIC_E_ARGUMENT, "%s: %s", F.reader, std::string(g_err).c_str()) : rc;
    Z.nl = L.nl;
    for (int l = 0; l < L.nl; l++) {
        rc = make_decode_geometry(w, h, L.g[l].B, L.g[l].wK, n_iso, 1, zoom, &Z.g[l]);
        if (rc) return rc;
    }
    if (n < 1 || n > L.g[L.nl - 1].Nr) return fail(FIC_E_ARGUMENT, "%s: %d leaves", F.reader, n);
    const int per = qt_run_ints(F, n_iso);
    const int64_t need = 4 * (kQtHeaderInts + per * (int64_t)n);
    if (len != need)
        return fail(FIC_E_ARGUMENT, "%s: %lld bytes, %d leaves need exactly %lld", F.reader, (long long)len, n, (long long)need);
    const uint8_t* rows = run + 4 * kQtHeaderInts;
    const int nq = F.QW - 1;                           // {qa, qb} / {q1, q2, q3, q4} behind {B, idx_local}
    // a leaf's level follows from its side, so every list has its exact size (zeros) before the walk fills it: a leaf reaches
    // emit at level l only with side B_max >> l, and at most once
    size_t count[kQtMaxLevels] = {0, 0, 0}, fill[kQtMaxLevels] = {0, 0, 0};
    for (int i = 0; i < n; i++) {
        const int b = get_be32(rows + 4 * per * (size_t)i);
        for (int l = 0; l < L.nl; l++) count[l] += b == L.g[l].B;
    }
    for (int l = 0; l < L.nl; l++) out->lv[l].resize(count[l] * F.dev_ints);
    int sqoff = 0;
    const bool ok = qt_tile(L, n, [&](int i) { return get_be32(rows + 4 * per * (size_t)i); }, [&](int i, int x, int y, int l) {
        const FicGeom& g = L.g[l];
        const uint8_t* r = rows + 4 * per * (size_t)i;
        const int idx = get_be32(r + 4), iso = per > 1 + F.QW ? get_be32(r + 4 * (1 + F.QW)) : 0;
        if (idx < 0 || idx >= g.wK * g.wK || iso < 0 || iso >= n_iso) return false;
        const int gi = host_window_to_global(g, (y / g.B) * g.Rw + x / g.B, idx);
        if (gi < 0 || gi >= g.Nd) return false;
        int32_t* e = &out->lv[l][fill[l]];
        fill[l] += F.dev_ints;
        e[0] = zoom * x; e[1] = zoom * y; e[2] = gi; e[3] = sqoff;
        for (int k = 0; k < nq; k++) e[4 + k] = get_be32(r + 8 + 4 * k);
        if (F.iso) e[8] = iso;
        if (grey) e[6] = iso;                          // q = {qa, qb, iso, 0}
        sqoff += Z.g[l].n;
        return true;
    });
    if (!ok)
        return fail(FIC_E_ARGUMENT, "%s: the leaf sizes do not tile the %dx%d image with levels %d..%d, or a leaf's domain index%s is "
                                    "out of range", F.reader, w, h, B_max, B_min, (grey || F.iso) ? " / isometry" : "");
    return FIC_OK;
}

}  // namespace ficd

using namespace ficd;

extern "C" {

const char* fic_last_error(void) { return g_err.c_str(); }
int fic_last_error_code(void) { return g_err_code; }

int64_t fic_write_run_gray(const int32_t* qrows, int n_ranges, int w, int h, int B, int wK, uint8_t* out, int64_t capacity)
{
    return write_fixed(kRunGrey, qrows, nullptr, n_ranges, w, h, B, wK, out, capacity);
}

int64_t fic_write_run_rgb(const int32_t* qrows5, int n_ranges, int w, int h, int B, int wK, uint8_t* out, int64_t capacity)
{
    return write_fixed(kRunRgb, qrows5, nullptr, n_ranges, w, h, B, wK, out, capacity);
}

int64_t fic_write_run_gray_iso(const int32_t* qrows, const int32_t* iso, int n_ranges, int w, int h, int B, int wK, uint8_t* out,
                               int64_t capacity)
{
    return write_fixed(kIsoGrey, qrows, iso, n_ranges, w, h, B, wK, out, capacity);
}

int64_t fic_write_run_rgb_iso(const int32_t* qrows5, const int32_t* iso, int n_ranges, int w, int h, int B, int wK, uint8_t* out,
                              int64_t capacity)
{
    return write_fixed(kIsoRgb, qrows5, iso, n_ranges, w, h, B, wK, out, capacity);
}

int64_t fic_write_run_quadtree(const int32_t* leaves, int n_leaves, int w, int h, int B_max, int B_min, int wK, int n_iso,
                               uint8_t* out, int64_t capacity)
{
    return write_quadtree(kQtGreyStream, leaves, n_leaves, w, h, B_max, B_min, wK, n_iso, out, capacity);
}

int64_t fic_write_run_rgb_quadtree(const int32_t* leaves, int n_leaves, int w, int h, int B_max, int B_min, int wK, uint8_t* out,
                                   int64_t capacity)
{
    return write_quadtree(kQtRgbStream, leaves, n_leaves, w, h, B_max, B_min, wK, 1, out, capacity);
}

int64_t fic_write_run_rgb_quadtree_iso(const int32_t* leaves, int n_leaves, int w, int h, int B_max, int B_min, int wK, uint8_t* out,
                                       int64_t capacity)
{
    return write_quadtree(kQtRgbIsoStream, leaves, n_leaves, w, h, B_max, B_min, wK, 8, out, capacity);
}

int64_t fic_quadtree_leaves_for_bytes(int tag, int n_iso, int64_t max_bytes)
{
    const QtFormat* F = nullptr;
    for (const QtFormat* f : {&kQtGreyStream, &kQtRgbStream, &kQtRgbIsoStream})
        if (f->tag == tag) F = f;
    if (!F) return fail(FIC_E_ARGUMENT, "fic_quadtree_leaves_for_bytes: tag %d is no quadtree stream (2, 3, 6)", tag);
    if ((n_iso != 1 && n_iso != 8) || (tag == 3 && n_iso != 1))
        return fail(FIC_E_ARGUMENT, "fic_quadtree_leaves_for_bytes: n_iso=%d for tag %d", n_iso, tag);
    if (max_bytes < 4 * kQtHeaderInts) return fail(FIC_E_CAPACITY, "%s: %lld bytes do not hold the 32-byte header", F->writer, (long long)max_bytes);
    return (max_bytes - 4 * kQtHeaderInts) / (4 * qt_run_ints(*F, n_iso));
}

}  // extern "C"
