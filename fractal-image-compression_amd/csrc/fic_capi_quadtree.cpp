// fic_capi_quadtree.cpp -- C ABI, quadtree (variable block size) codec, grey and joint RGB: encode every level with the
// one-shot machinery, collage SSE + split + compaction on the device (fic_quadtree.hip), and the decoders of leaves of mixed
// size on the decode job (fic_internal.h).  The tag-2 (grey), tag-3 (colour) and tag-6 (colour with an isometry column) stream
// writers and parsers are in fic_stream.cpp.  Host-side orchestration only.  Semantics: DESIGN.md sections 4.13 (grey), 4.14
// (colour), 4.17 (colour with the 8 isometries) and 4.18 (encode to a leaf budget).
#include "fic_internal.h"

using namespace ficd;

namespace {

// ---- the host side of a pixel format (QtGrey / QtRgb / QtRgbIso, fic_launch.h) --------------------------------------------
// The one-shot contexts an encode runs its levels through, their device buffers and the stream format (fic_stream.h).
template <typename Px>
struct QtViews {
    const Px *image, *scaled;         // the input [H][W] and the 2:1 copy [Hs][Ws] the rows refer to
    const int32_t *qrows, *iso;
};

struct QtGreyHost : QtGrey {
    using Dev = QtGrey;               // the tag of the launchers
    using Ctx = fic_ctx;
    static constexpr const QtFormat& kStream = kQtGreyStream;
    static constexpr const DecodeKind& kDecode = kDecodeGrey;
    static Ctx* take(int device, const FicGeom& g)
    {
        Ctx* c = g_idle_grey.take(device, g.W, g.H, g.B, g.wK, g.n_iso);
        return c ? c : fic_ctx_create(device, g.W, g.H, g.B, g.wK, g.n_iso, 1);
    }
    static int encode(Ctx* c, const uint8_t* gray, const int32_t* argb, int search)   // exactly the one-shot encode of this level
    {
        int rc = gray ? fic_ctx_set_gray_host(c, gray) : fic_ctx_set_argb_host(c, argb);
        if (rc || !search) return rc ? rc : fic_ctx_encode(c, 0, -1, nullptr);
        // least squares: the cached context goes back in the reference's mode whatever happens
        rc = fic_ctx_set_option(c, "search", search);
        if (rc == FIC_OK) rc = fic_ctx_encode(c, 0, -1, nullptr);
        ErrKeep keep;
        (void)fic_ctx_set_option(c, "search", 0);
        return rc;
    }
    static void give(Ctx* c, bool ok) { ok ? g_idle_grey.give(c) : fic_ctx_destroy(c); }
    // every level reads the top context's scaled copy, made here: the original, 2:1 scaled (FC:970-1007)
    static int prepare(Ctx* top) { return fic_launch_scale(top->b.gray, top->b.scaled, top->g, nullptr); }
    static QtViews<Px> views(const Ctx* c, const Ctx* top) { return {c->b.gray, top->b.scaled, c->o.qrows, c->g.n_iso > 1 ? c->o.iso : nullptr}; }
    static int scale(const Px* image, Px* scaled, const FicGeom& g) { return fic_launch_scale(image, scaled, g, nullptr); }
};

struct QtRgbHost : QtRgb {
    using Dev = QtRgb;
    using Ctx = fic_rgb_ctx;
    static constexpr const QtFormat& kStream = kQtRgbStream;
    static constexpr const DecodeKind& kDecode = kDecodeRgb;
    static Ctx* take(int device, const FicGeom& g)
    {
        Ctx* c = g_idle_rgb.take(device, g.W, g.H, g.B, g.wK, 1);
        return c ? c : fic_rgb_ctx_create(device, g.W, g.H, g.B, g.wK, 1);
    }
    static int encode(Ctx* c, const uint8_t*, const int32_t* argb, int search = 0)   // exactly the one-shot RGB encode of this level
    {
        int rc = fic_rgb_ctx_set_argb_host(c, argb);
        if (rc || !search) return rc ? rc : fic_rgb_ctx_encode(c, 0, nullptr);
        // least squares: the cached context goes back in the reference's mode whatever happens
        rc = fic_rgb_ctx_set_option(c, "search", search);
        if (rc == FIC_OK) rc = fic_rgb_ctx_encode(c, 0, nullptr);
        ErrKeep keep;
        (void)fic_rgb_ctx_set_option(c, "search", 0);
        return rc;
    }
    static void give(Ctx* c, bool ok) { ok ? g_idle_rgb.give(c) : fic_rgb_ctx_destroy(c); }
    static int prepare(Ctx*) { return 0; }
    // every level reads its own scaleImageRGB copy, made by its encode (image 0 of the context)
    static QtViews<Px> views(const Ctx* c, const Ctx*) { return {c->argb, c->scaled, c->qrows, nullptr}; }
    static int scale(const Px* image, Px* scaled, const FicGeom& g) { return fic_launch_scale_rgb(image, scaled, g, nullptr); }
};

// Colour with an isometry column: the joint-RGB contexts of n_iso = 1 or 8, tag 6.  The stream always holds
// the column (zeros for an n_iso = 1 codebook) and its reader takes every isometry 0..7.
struct QtRgbIsoHost : QtRgbIso {
    using Dev = QtRgbIso;
    using Ctx = fic_rgb_ctx;
    static constexpr const QtFormat& kStream = kQtRgbIsoStream;
    static constexpr const DecodeKind& kDecode = kDecodeRgb;
    static Ctx* take(int device, const FicGeom& g)
    {
        Ctx* c = g_idle_rgb.take(device, g.W, g.H, g.B, g.wK, g.n_iso);
        return c ? c : fic_rgb_ctx_create_iso(device, g.W, g.H, g.B, g.wK, g.n_iso, 1);
    }
    static int encode(Ctx* c, const uint8_t* gray, const int32_t* argb, int search = 0) { return QtRgbHost::encode(c, gray, argb, search); }   // = fic_encode_rgb_iso_argb's / _lsq_argb's
    static void give(Ctx* c, bool ok) { QtRgbHost::give(c, ok); }
    static int prepare(Ctx*) { return 0; }
    static QtViews<Px> views(const Ctx* c, const Ctx*) { return {c->argb, c->scaled, c->qrows, c->iso}; }   // iso NULL on n_iso = 1: the identity
    static int scale(const Px* image, Px* scaled, const FicGeom& g) { return fic_launch_scale_rgb(image, scaled, g, nullptr); }
};

// Encode to a leaf budget: the threshold is chosen on the device, from the SSE arrays of this encode, as the
// smallest float whose tree has at most max_leaves leaves.
struct QtBudget {
    int64_t max_leaves;
    float* threshold_out;    // the threshold chosen (also set on FIC_E_CAPACITY)
    uint64_t* stats4;        // NULL or {collage SSE of the leaves, leaves of side B_max, B_max / 2, B_max / 4}
};

// Encode by rate-distortion pruning: the tree that minimises D + lambda N, lambda given (goal 0) or chosen on
// the device from the SSE arrays of this encode: the smallest whose tree has at most `value` leaves (goal 1), or the smallest
// that gives the tree of fewest leaves with a collage SSE <= `value` (goal 2).
struct QtRd {
    int goal;
    uint64_t value;
    uint32_t* lambda_out;    // the lambda in force (also set on FIC_E_CAPACITY)
    uint64_t* stats4;        // as QtBudget's
};

// The encode behind fic_encode_*_quadtree_* and the SSE test hooks: every level through the one-shot contexts, then the
// per-level SSE, the split and the compaction on the device.  leaves / sse_out may be NULL.  budget: NULL, or the threshold
// comes from the budget's select instead of the argument.  rd: NULL, or the split rule is "e(v) > lambda" on the keys of the
// pruning instead of the threshold's.  search: the criterion of the per-level codebooks (0 the
// reference's, 1 least squares: DESIGN.md 4.19 grey, 4.20 colour); everything after them is the same code.
template <typename Fmt>
int qt_encode(const uint8_t* gray, const int32_t* argb, int w, int h, int B_max, int B_min, int wK, int n_iso, float threshold,
              int device, int32_t* leaves, int64_t capacity, int* n_leaves, uint32_t* sse_out, int64_t sse_capacity,
              const QtBudget* budget = nullptr, int search = 0, const QtRd* rd = nullptr)
{
    if (!gray && !argb) return fail(FIC_E_ARGUMENT, "%s encode: null image", Fmt::kStream.kind);
    if (threshold != threshold) return fail(FIC_E_ARGUMENT, "%s encode: threshold is NaN", Fmt::kStream.kind);
    QtLevels L;
    int rc = qt_levels(w, h, B_max, B_min, wK, n_iso, &L);
    if (rc) return rc;
    if (budget && budget->max_leaves < L.g[0].Nr)
        return fail(FIC_E_ARGUMENT, "%s encode: max_leaves = %lld, the image has %d blocks of side %d", Fmt::kStream.kind,
                    (long long)budget->max_leaves, L.g[0].Nr, B_max);
    if (rd && rd->goal == FIC_QT_RD_LEAVES && rd->value < (uint64_t)L.g[0].Nr)
        return fail(FIC_E_ARGUMENT, "%s encode: max_leaves = %llu, the image has %d blocks of side %d", Fmt::kStream.kind,
                    (unsigned long long)rd->value, L.g[0].Nr, B_max);
    size_t sse_total = 0;
    for (int l = 0; l < L.nl; l++) sse_total += (size_t)L.g[l].Nr;
    if (sse_out && sse_capacity < (int64_t)sse_total)
        return fail(FIC_E_CAPACITY, "%s SSE: need %zu values, have %lld", Fmt::kStream.kind, sse_total, (long long)sse_capacity);
    rc = check_device(device);
    if (rc) return rc;

    typename Fmt::Ctx* c[kQtMaxLevels] = {nullptr, nullptr, nullptr};
    DevMem mem(device);              // the scratch of this call: freed on every way out
    char* scratch = nullptr;
    for (int l = 0; l < L.nl && rc == FIC_OK; l++) {
        c[l] = Fmt::take(device, L.g[l]);
        if (!c[l]) { rc = g_err_code ? g_err_code : FIC_E_HIP; break; }
        rc = Fmt::encode(c[l], gray, argb, search);
    }
    // scratch: SSE per level, counts / offsets per top-level block, the leaf table (room for every block of B_min)
    const FicGeom& top = L.g[0];
    const size_t max_leaves = (size_t)L.g[L.nl - 1].Nr;
    size_t o_sse[kQtMaxLevels], off = 0;
    for (int l = 0; l < L.nl; l++) { o_sse[l] = off; off += align256((size_t)L.g[l].Nr * 4); }
    const size_t o_cnt = off, o_offs = o_cnt + align256((size_t)top.Nr * 4), o_leaves = o_offs + align256(((size_t)top.Nr + 1) * 4);
    // a budget: the split keys of every block above B_min, the select's histograms and result, the tree's statistics
    const int n1 = L.nl == 3 ? L.g[1].Nr : 0, nkeys = top.Nr + n1;
    // pruning: the same and the gains G_v; the statistics' 256 bytes also hold the top-level SSE sum (+64) and a given lambda (+128)
    static_assert(FIC_QT_SELECT_W_WORDS * 8 >= FIC_QT_SELECT_WORDS * 4, "one select area for both selects");
    const size_t o_keys = o_leaves + align256(max_leaves * Fmt::kLeafInts * 4), o_gains = o_keys + (budget || rd ? align256((size_t)nkeys * 4) : 0),
                 o_sel = o_gains + (rd ? align256((size_t)nkeys * 8) : 0),
                 o_stats = o_sel + (rd ? align256(FIC_QT_SELECT_W_WORDS * 8) : (budget ? align256(FIC_QT_SELECT_WORDS * 4) : 0)),
                 total = o_stats + (budget || rd ? 256 : 0);
    if (rc == FIC_OK) rc = mem.alloc(scratch, total);
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
    if (rc == FIC_OK && budget) {
        // rank S = (M - Ntop) / 3 in descending order: the S blocks of larger key may split, the block of rank S must not
        const int64_t S = (budget->max_leaves - top.Nr) / 3;
        uint32_t* d_sel = (uint32_t*)(scratch + o_sel);
        if (fic_launch_qt_keys(sse, Rw, L.nl, top.B, top.Rw, top.Nr, n1, (uint32_t*)(scratch + o_keys), nullptr) ||
            fic_launch_qt_select((const uint32_t*)(scratch + o_keys), (uint32_t)nkeys, (uint32_t)(S < nkeys ? S : nkeys), d_sel, nullptr))
            rc = fail(FIC_E_HIP, "%s budget select launch failed", Fmt::kStream.kind);
        if (rc == FIC_OK) {     // by value into the compaction, like n below; the caller gets it anyway
            hipError_t e = hipMemcpy(&threshold, d_sel + 4 * 256 + 1, sizeof(float), hipMemcpyDeviceToHost);
            if (e != hipSuccess) rc = fail(FIC_E_HIP, "%s encode: %s", Fmt::kStream.kind, hipGetErrorString(e));
            else *budget->threshold_out = threshold;
        }
    }
    const uint32_t *d_keys = (const uint32_t*)(scratch + o_keys), *d_lambda = nullptr;
    if (rc == FIC_OK && rd) {
        unsigned long long* d_top = (unsigned long long*)(scratch + o_stats + 64);
        if (fic_launch_qt_rd_keys(sse, Rw, L.nl, top.B, top.Rw, top.Nr, n1, (uint32_t*)(scratch + o_keys), (long long*)(scratch + o_gains), d_top, nullptr))
            rc = fail(FIC_E_HIP, "%s pruning keys launch failed", Fmt::kStream.kind);
        uint32_t lambda = (uint32_t)rd->value;
        if (rc == FIC_OK && rd->goal == FIC_QT_RD_LAMBDA) {
            d_lambda = (const uint32_t*)(scratch + o_stats + 128);
            hipError_t e = hipMemsetD32Async((hipDeviceptr_t)(scratch + o_stats + 128), (int)lambda, 1, nullptr);
            if (e != hipSuccess) rc = fail(FIC_E_HIP, "%s encode: %s", Fmt::kStream.kind, hipGetErrorString(e));
        } else if (rc == FIC_OK) {
            int bad;
            if (rd->goal == FIC_QT_RD_LEAVES) {       // the select of 4.18 on the new keys, rank S = (M - Ntop) / 3
                const uint64_t S = (rd->value - (uint64_t)top.Nr) / 3;
                uint32_t* d_sel = (uint32_t*)(scratch + o_sel);
                bad = fic_launch_qt_select(d_keys, (uint32_t)nkeys, (uint32_t)(S < (uint64_t)nkeys ? S : (uint64_t)nkeys), d_sel, nullptr);
                d_lambda = d_sel + 4 * 256;
            } else {                                  // the summed gain has to reach sum S_top - max_sse
                unsigned long long* d_sel = (unsigned long long*)(scratch + o_sel);
                const uint64_t cap = (uint64_t)INT64_MAX;
                bad = fic_launch_qt_select_w(d_keys, (const long long*)(scratch + o_gains), (uint32_t)nkeys, d_top,
                                             (long long)(rd->value < cap ? rd->value : cap), d_sel, nullptr);
                d_lambda = (const uint32_t*)(d_sel + 4 * 256);
            }
            if (bad) rc = fail(FIC_E_HIP, "%s pruning select launch failed", Fmt::kStream.kind);
            if (rc == FIC_OK) {     // the caller's copy; the walkers read it where it is
                hipError_t e = hipMemcpy(&lambda, d_lambda, sizeof(uint32_t), hipMemcpyDeviceToHost);
                if (e != hipSuccess) rc = fail(FIC_E_HIP, "%s encode: %s", Fmt::kStream.kind, hipGetErrorString(e));
            }
        }
        if (rc == FIC_OK) *rd->lambda_out = lambda;
    }
    int* d_offs = (int*)(scratch + o_offs);
    if (rc == FIC_OK && (rd ? fic_launch_qt_compact_rd<typename Fmt::Dev>(sse, qrows, iso, Rw, L.nl, top.B, top.Rw, top.Nr, d_keys, d_lambda,
                                                                          (int*)(scratch + o_cnt), d_offs, (int32_t*)(scratch + o_leaves), nullptr)
                            : fic_launch_qt_compact<typename Fmt::Dev>(sse, qrows, iso, Rw, L.nl, top.B, top.Rw, top.Nr, threshold,
                                                                       (int*)(scratch + o_cnt), d_offs, (int32_t*)(scratch + o_leaves), nullptr)))
        rc = fail(FIC_E_HIP, "%s compaction launch failed", Fmt::kStream.kind);
    int n = 0;
    if (rc == FIC_OK) {
        hipError_t e = hipMemcpy(&n, d_offs + top.Nr, sizeof(int), hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(FIC_E_HIP, "%s encode: %s", Fmt::kStream.kind, hipGetErrorString(e));
    }
    if (rc == FIC_OK && n_leaves) *n_leaves = n;
    uint64_t* stats4 = budget ? budget->stats4 : (rd ? rd->stats4 : nullptr);
    if (rc == FIC_OK && stats4) {
        static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "stats4");
        if (rd ? fic_launch_qt_tree_stats_rd(sse, Rw, L.nl, top.B, top.Rw, top.Nr, d_keys, d_lambda, (unsigned long long*)(scratch + o_stats), nullptr)
               : fic_launch_qt_tree_stats(sse, Rw, L.nl, top.B, top.Rw, top.Nr, threshold, (unsigned long long*)(scratch + o_stats), nullptr))
            rc = fail(FIC_E_HIP, "%s tree statistics launch failed", Fmt::kStream.kind);
        else {
            hipError_t e = hipMemcpy(stats4, scratch + o_stats, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost);
            if (e != hipSuccess) rc = fail(FIC_E_HIP, "%s encode: %s", Fmt::kStream.kind, hipGetErrorString(e));
        }
    }
    if (rc == FIC_OK && leaves) {
        if (capacity < n) rc = fail(FIC_E_CAPACITY, "%s encode: %d leaves, room for %lld", Fmt::kStream.kind, n, (long long)capacity);
        else {
            hipError_t e = hipMemcpy(leaves, scratch + o_leaves, (size_t)n * Fmt::kLeafInts * 4, hipMemcpyDeviceToHost);
            if (e != hipSuccess) rc = fail(FIC_E_HIP, "%s encode: %s", Fmt::kStream.kind, hipGetErrorString(e));
        }
    }
    for (int l = 0, o = 0; rc == FIC_OK && sse_out && l < L.nl; o += L.g[l].Nr, l++) {
        hipError_t e = hipMemcpy(sse_out + o, scratch + o_sse[l], (size_t)L.g[l].Nr * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(FIC_E_HIP, "%s SSE: %s", Fmt::kStream.kind, hipGetErrorString(e));
    }
    ErrKeep keep;
    for (int l = 0; l < L.nl; l++)
        if (c[l]) Fmt::give(c[l], rc == FIC_OK);
    return rc;
}

// The stream decoder: the parsed leaves of every level uploaded, then the decoder's loop with one paint per level and iteration.
template <typename Fmt>
int qt_decode_run(const uint8_t* run, int64_t len, int zoom, int device, typename Fmt::Px* out, int64_t capacity_pixels, int* w_out, int* h_out,
                  float* avg_error_io, int* iterations)
{
    using Leaf = typename Fmt::Leaf;
    const QtFormat& F = Fmt::kStream;
    static_assert(sizeof(Leaf) == Fmt::kStream.dev_ints * sizeof(int32_t) && Fmt::kLeafInts == Fmt::kStream.leaf_ints, "the parser's leaf layout");
    QtStream S;
    int rc = parse_quadtree(F, run, len, zoom, &S);
    if (rc) return rc;
    const FicGeom& g0 = S.Z.g[0];
    if (w_out) *w_out = g0.W;
    if (h_out) *h_out = g0.H;
    const size_t npix = (size_t)g0.W * g0.H;
    if (!out || capacity_pixels < (int64_t)npix) return fail(FIC_E_CAPACITY, "%s: output needs %zu pixels", F.reader, npix);
    rc = check_device(device);
    if (rc) return rc;
    DecodeJob J;
    rc = J.open(F.reader, device, Fmt::kDecode, g0, nullptr, {&S.lv[0], &S.lv[1], &S.lv[2]});
    if (rc) return rc;
    typename Fmt::Px *d_scaled = (typename Fmt::Px*)J.scaled, *d_image = (typename Fmt::Px*)J.image;
    // one iteration: scale the current image (FC:382, FC:459), paint the leaves level by level from that copy, loop control
    return J.run(F.reader, avg_error_io, avg_error_io, iterations, nullptr, out, [&](int counter) {
        if (Fmt::scale(d_image, d_scaled, g0)) return -1;
        for (int l = 0; l < S.Z.nl; l++)
            if (fic_launch_decode_paint_leaves<typename Fmt::Dev>(d_scaled, d_image, (const Leaf*)J.spans[l], (int)(S.lv[l].size() / F.dev_ints),
                                                                  J.state, J.sq, counter, S.Z.g[l], nullptr))
                return -1;
        return fic_launch_decode_step(J.state, J.sq, counter, (int)npix, 1, nullptr);
    });
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

int fic_encode_gray_quadtree_lsq_u8(const uint8_t* gray, int w, int h, int B_max, int B_min, int wK, int n_iso, float threshold,
                                    int device, int32_t* leaves, int64_t capacity, int* n_leaves)
{
    if (!gray || !leaves || !n_leaves) return fail(FIC_E_ARGUMENT, "fic_encode_gray_quadtree_lsq_u8: null argument");
    return qt_encode<QtGreyHost>(gray, nullptr, w, h, B_max, B_min, wK, n_iso, threshold, device, leaves, capacity, n_leaves, nullptr, 0, nullptr, 1);
}

int fic_encode_gray_quadtree_lsq_argb(const int32_t* argb, int w, int h, int B_max, int B_min, int wK, int n_iso, float threshold,
                                      int device, int32_t* leaves, int64_t capacity, int* n_leaves)
{
    if (!argb || !leaves || !n_leaves) return fail(FIC_E_ARGUMENT, "fic_encode_gray_quadtree_lsq_argb: null argument");
    return qt_encode<QtGreyHost>(nullptr, argb, w, h, B_max, B_min, wK, n_iso, threshold, device, leaves, capacity, n_leaves, nullptr, 0, nullptr, 1);
}

int fic_encode_gray_quadtree_budget_u8(const uint8_t* gray, int w, int h, int B_max, int B_min, int wK, int n_iso, int64_t max_leaves,
                                       int device, int32_t* leaves, int64_t capacity, int* n_leaves, float* threshold_out, uint64_t* stats4)
{
    if (!gray || !leaves || !n_leaves || !threshold_out) return fail(FIC_E_ARGUMENT, "fic_encode_gray_quadtree_budget_u8: null argument");
    const QtBudget b{max_leaves, threshold_out, stats4};
    return qt_encode<QtGreyHost>(gray, nullptr, w, h, B_max, B_min, wK, n_iso, 0.0f, device, leaves, capacity, n_leaves, nullptr, 0, &b);
}

int fic_encode_gray_quadtree_budget_argb(const int32_t* argb, int w, int h, int B_max, int B_min, int wK, int n_iso, int64_t max_leaves,
                                         int device, int32_t* leaves, int64_t capacity, int* n_leaves, float* threshold_out, uint64_t* stats4)
{
    if (!argb || !leaves || !n_leaves || !threshold_out) return fail(FIC_E_ARGUMENT, "fic_encode_gray_quadtree_budget_argb: null argument");
    const QtBudget b{max_leaves, threshold_out, stats4};
    return qt_encode<QtGreyHost>(nullptr, argb, w, h, B_max, B_min, wK, n_iso, 0.0f, device, leaves, capacity, n_leaves, nullptr, 0, &b);
}

// Test hook: the select of an encode to a budget (k_qt_select_hist x 4, k_qt_select_final) on the caller's keys
int fic_debug_qt_select(int device, const uint32_t* keys, int64_t n, int64_t rank, uint32_t* key_out, float* threshold_out, int64_t* above_out)
{
    if (!keys || !key_out || !threshold_out || !above_out) return fail(FIC_E_ARGUMENT, "fic_debug_qt_select: null argument");
    if (n < 1 || n >= 0x7FFFFFFFll || rank < 0) return fail(FIC_E_ARGUMENT, "fic_debug_qt_select: n = %lld, rank = %lld", (long long)n, (long long)rank);
    int rc = check_device(device);
    if (rc) return rc;
    DevMem mem(device);
    char* scratch = nullptr;
    const size_t o_sel = align256((size_t)n * 4);
    rc = mem.alloc(scratch, o_sel + FIC_QT_SELECT_WORDS * 4);
    if (rc) return rc;
    uint32_t res[4] = {0, 0, 0, 0};
    hipError_t e = hipMemcpy(scratch, keys, (size_t)n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && fic_launch_qt_select((const uint32_t*)scratch, (uint32_t)n, (uint32_t)(rank < n ? rank : n), (uint32_t*)(scratch + o_sel), nullptr))
        return fail(FIC_E_HIP, "fic_debug_qt_select: launch failed");
    if (e == hipSuccess) e = hipMemcpy(res, scratch + o_sel + 4 * 256 * 4, sizeof(res), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(FIC_E_HIP, "fic_debug_qt_select: %s", hipGetErrorString(e));
    *key_out = res[0];
    memcpy(threshold_out, &res[1], sizeof(float));
    *above_out = res[2];
    return FIC_OK;
}

int fic_debug_quadtree_sse(const uint8_t* gray, int w, int h, int B_max, int B_min, int wK, int n_iso, int device, uint32_t* sse,
                           int64_t capacity)
{
    if (!gray || !sse) return fail(FIC_E_ARGUMENT, "fic_debug_quadtree_sse: null argument");
    return qt_encode<QtGreyHost>(gray, nullptr, w, h, B_max, B_min, wK, n_iso, __builtin_inff(), device, nullptr, 0, nullptr, sse, capacity);
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

int fic_encode_rgb_quadtree_lsq_argb(const int32_t* argb, int w, int h, int B_max, int B_min, int wK, float threshold, int device,
                                     int32_t* leaves, int64_t capacity, int* n_leaves)
{
    if (!argb || !leaves || !n_leaves) return fail(FIC_E_ARGUMENT, "fic_encode_rgb_quadtree_lsq_argb: null argument");
    return qt_encode<QtRgbHost>(nullptr, argb, w, h, B_max, B_min, wK, 1, threshold, device, leaves, capacity, n_leaves, nullptr, 0, nullptr, 1);
}

int fic_encode_rgb_quadtree_budget_argb(const int32_t* argb, int w, int h, int B_max, int B_min, int wK, int64_t max_leaves, int device,
                                        int32_t* leaves, int64_t capacity, int* n_leaves, float* threshold_out, uint64_t* stats4)
{
    if (!argb || !leaves || !n_leaves || !threshold_out) return fail(FIC_E_ARGUMENT, "fic_encode_rgb_quadtree_budget_argb: null argument");
    const QtBudget b{max_leaves, threshold_out, stats4};
    return qt_encode<QtRgbHost>(nullptr, argb, w, h, B_max, B_min, wK, 1, 0.0f, device, leaves, capacity, n_leaves, nullptr, 0, &b);
}

int fic_debug_rgb_quadtree_sse(const int32_t* argb, int w, int h, int B_max, int B_min, int wK, int device, uint32_t* sse,
                               int64_t capacity)
{
    if (!argb || !sse) return fail(FIC_E_ARGUMENT, "fic_debug_rgb_quadtree_sse: null argument");
    return qt_encode<QtRgbHost>(nullptr, argb, w, h, B_max, B_min, wK, 1, __builtin_inff(), device, nullptr, 0, nullptr, sse, capacity);
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

int fic_encode_rgb_quadtree_iso_lsq_argb(const int32_t* argb, int w, int h, int B_max, int B_min, int wK, int n_iso, float threshold,
                                         int device, int32_t* leaves, int64_t capacity, int* n_leaves)
{
    if (!argb || !leaves || !n_leaves) return fail(FIC_E_ARGUMENT, "fic_encode_rgb_quadtree_iso_lsq_argb: null argument");
    return qt_encode<QtRgbIsoHost>(nullptr, argb, w, h, B_max, B_min, wK, n_iso, threshold, device, leaves, capacity, n_leaves, nullptr, 0, nullptr, 1);
}

int fic_encode_rgb_quadtree_iso_budget_argb(const int32_t* argb, int w, int h, int B_max, int B_min, int wK, int n_iso, int64_t max_leaves,
                                            int device, int32_t* leaves, int64_t capacity, int* n_leaves, float* threshold_out,
                                            uint64_t* stats4)
{
    if (!argb || !leaves || !n_leaves || !threshold_out) return fail(FIC_E_ARGUMENT, "fic_encode_rgb_quadtree_iso_budget_argb: null argument");
    const QtBudget b{max_leaves, threshold_out, stats4};
    return qt_encode<QtRgbIsoHost>(nullptr, argb, w, h, B_max, B_min, wK, n_iso, 0.0f, device, leaves, capacity, n_leaves, nullptr, 0, &b);
}

int fic_debug_rgb_quadtree_iso_sse(const int32_t* argb, int w, int h, int B_max, int B_min, int wK, int n_iso, int device,
                                   uint32_t* sse, int64_t capacity)
{
    if (!argb || !sse) return fail(FIC_E_ARGUMENT, "fic_debug_rgb_quadtree_iso_sse: null argument");
    return qt_encode<QtRgbIsoHost>(nullptr, argb, w, h, B_max, B_min, wK, n_iso, __builtin_inff(), device, nullptr, 0, nullptr, sse, capacity);
}

int fic_decode_rgb_quadtree_iso_run(const uint8_t* run, int64_t len, int zoom, int device, int32_t* argb_out, int64_t capacity_pixels,
                                    int* w_out, int* h_out, float* avg_error_io, int* iterations)
{
    return qt_decode_run<QtRgbIsoHost>(run, len, zoom, device, argb_out, capacity_pixels, w_out, h_out, avg_error_io, iterations);
}

}  // extern "C"

// ---- encode by rate-distortion pruning -------------------------------------------------------------------
namespace {

// The checks of an RD entry that need no geometry; the ladder, the window and max_leaves >= N_top follow in qt_encode, all
// before any device work.
template <typename Fmt>
int qt_encode_rd(const char* entry, const uint8_t* gray, const int32_t* argb, int w, int h, int B_max, int B_min, int wK, int n_iso, int search,
                 int goal, uint64_t value, int device, int32_t* leaves, int64_t capacity, int* n_leaves, uint32_t* lambda_out, uint64_t* stats4)
{
    if ((!gray && !argb) || !leaves || !n_leaves || !lambda_out) return fail(FIC_E_ARGUMENT, "%s: null argument", entry);
    if (goal < FIC_QT_RD_LAMBDA || goal > FIC_QT_RD_SSE) return fail(FIC_E_ARGUMENT, "%s: goal = %d, need 0 (lambda), 1 (leaves) or 2 (SSE)", entry, goal);
    if (search != 0 && search != 1) return fail(FIC_E_ARGUMENT, "%s: search = %d, need 0 (reference) or 1 (least squares)", entry, search);
    if (goal == FIC_QT_RD_LAMBDA && value > 0xFFFFFFFFull)
        return fail(FIC_E_ARGUMENT, "%s: lambda = %llu, need 0 .. 2^32 - 1", entry, (unsigned long long)value);
    const QtRd rd{goal, value, lambda_out, stats4};
    return qt_encode<Fmt>(gray, argb, w, h, B_max, B_min, wK, n_iso, 0.0f, device, leaves, capacity, n_leaves, nullptr, 0, nullptr, search, &rd);
}

}  // namespace

extern "C" {

int fic_encode_gray_quadtree_rd_u8(const uint8_t* gray, int w, int h, int B_max, int B_min, int wK, int n_iso, int search, int goal,
                                   uint64_t value, int device, int32_t* leaves, int64_t capacity, int* n_leaves, uint32_t* lambda_out,
                                   uint64_t* stats4)
{
    return qt_encode_rd<QtGreyHost>("fic_encode_gray_quadtree_rd_u8", gray, nullptr, w, h, B_max, B_min, wK, n_iso, search, goal, value, device,
                                    leaves, capacity, n_leaves, lambda_out, stats4);
}

int fic_encode_gray_quadtree_rd_argb(const int32_t* argb, int w, int h, int B_max, int B_min, int wK, int n_iso, int search, int goal,
                                     uint64_t value, int device, int32_t* leaves, int64_t capacity, int* n_leaves, uint32_t* lambda_out,
                                     uint64_t* stats4)
{
    return qt_encode_rd<QtGreyHost>("fic_encode_gray_quadtree_rd_argb", nullptr, argb, w, h, B_max, B_min, wK, n_iso, search, goal, value, device,
                                    leaves, capacity, n_leaves, lambda_out, stats4);
}

int fic_encode_rgb_quadtree_rd_argb(const int32_t* argb, int w, int h, int B_max, int B_min, int wK, int search, int goal, uint64_t value,
                                    int device, int32_t* leaves, int64_t capacity, int* n_leaves, uint32_t* lambda_out, uint64_t* stats4)
{
    return qt_encode_rd<QtRgbHost>("fic_encode_rgb_quadtree_rd_argb", nullptr, argb, w, h, B_max, B_min, wK, 1, search, goal, value, device, leaves,
                                   capacity, n_leaves, lambda_out, stats4);
}

int fic_encode_rgb_quadtree_iso_rd_argb(const int32_t* argb, int w, int h, int B_max, int B_min, int wK, int n_iso, int search, int goal,
                                        uint64_t value, int device, int32_t* leaves, int64_t capacity, int* n_leaves, uint32_t* lambda_out,
                                        uint64_t* stats4)
{
    return qt_encode_rd<QtRgbIsoHost>("fic_encode_rgb_quadtree_iso_rd_argb", nullptr, argb, w, h, B_max, B_min, wK, n_iso, search, goal, value,
                                      device, leaves, capacity, n_leaves, lambda_out, stats4);
}

// Test hook: k_qt_rd_keys on the caller's SSE arrays (the levels concatenated, as fic_debug_quadtree_sse returns them)
int fic_debug_qt_rd_keys(int device, const uint32_t* sse, int w, int h, int B_max, int B_min, uint32_t* keys, int64_t* gains)
{
    if (!sse || !keys || !gains) return fail(FIC_E_ARGUMENT, "fic_debug_qt_rd_keys: null argument");
    if (!((B_max == 8 || B_max == 16) && (B_min == 4 || B_min == 8) && B_min < B_max))
        return fail(FIC_E_ARGUMENT, "fic_debug_qt_rd_keys: levels B_max=%d B_min=%d", B_max, B_min);
    if (w <= 0 || h <= 0 || (w % B_max) || (h % B_max) || (int64_t)(w / B_min) * (h / B_min) >= 0x7FFFFFFFll)
        return fail(FIC_E_GEOMETRY, "fic_debug_qt_rd_keys: image %dx%d, B_max=%d", w, h, B_max);
    int rc = check_device(device);
    if (rc) return rc;
    int nl = 0, Rw[kQtMaxLevels], Nr[kQtMaxLevels];
    size_t o_sse[kQtMaxLevels], off = 0;
    for (int B = B_max; B >= B_min; B /= 2, nl++) {
        Rw[nl] = w / B;
        Nr[nl] = (w / B) * (h / B);
        o_sse[nl] = off;
        off += (size_t)Nr[nl] * 4;      // concatenated, like the caller's: one copy
    }
    const int n1 = nl == 3 ? Nr[1] : 0, nkeys = Nr[0] + n1;
    const size_t o_keys = align256(off), o_gains = o_keys + align256((size_t)nkeys * 4), o_top = o_gains + align256((size_t)nkeys * 8);
    DevMem mem(device);
    char* scratch = nullptr;
    rc = mem.alloc(scratch, o_top + 256);
    if (rc) return rc;
    const uint32_t* lv[kQtMaxLevels] = {nullptr, nullptr, nullptr};
    for (int l = 0; l < nl; l++) lv[l] = (const uint32_t*)(scratch + o_sse[l]);
    hipError_t e = hipMemcpy(scratch, sse, off, hipMemcpyHostToDevice);
    if (e == hipSuccess && fic_launch_qt_rd_keys(lv, Rw, nl, B_max, Rw[0], Nr[0], n1, (uint32_t*)(scratch + o_keys), (long long*)(scratch + o_gains),
                                                 (unsigned long long*)(scratch + o_top), nullptr))
        return fail(FIC_E_HIP, "fic_debug_qt_rd_keys: launch failed");
    if (e == hipSuccess) e = hipMemcpy(keys, scratch + o_keys, (size_t)nkeys * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(gains, scratch + o_gains, (size_t)nkeys * 8, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(FIC_E_HIP, "fic_debug_qt_rd_keys: %s", hipGetErrorString(e));
    return FIC_OK;
}

// Test hook: the weighted select (k_qt_select_hist_w x 4, k_qt_select_final_w) on the caller's keys and gains
int fic_debug_qt_select_weighted(int device, const uint32_t* keys, const int64_t* gains, int64_t n, int64_t need, uint32_t* key_out,
                                 int64_t* above_out, int64_t* gain_out)
{
    if (!keys || !gains || !key_out || !above_out || !gain_out) return fail(FIC_E_ARGUMENT, "fic_debug_qt_select_weighted: null argument");
    if (n < 1 || n >= 0x7FFFFFFFll) return fail(FIC_E_ARGUMENT, "fic_debug_qt_select_weighted: n = %lld", (long long)n);
    int rc = check_device(device);
    if (rc) return rc;
    static_assert(sizeof(long long) == sizeof(int64_t), "gains");
    DevMem mem(device);
    char* scratch = nullptr;
    const size_t o_gains = align256((size_t)n * 4), o_sel = o_gains + align256((size_t)n * 8);
    rc = mem.alloc(scratch, o_sel + FIC_QT_SELECT_W_WORDS * 8);
    if (rc) return rc;
    uint64_t res[4] = {0, 0, 0, 0};
    hipError_t e = hipMemcpy(scratch, keys, (size_t)n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(scratch + o_gains, gains, (size_t)n * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess && fic_launch_qt_select_w((const uint32_t*)scratch, (const long long*)(scratch + o_gains), (uint32_t)n, nullptr,
                                                  (long long)need, (unsigned long long*)(scratch + o_sel), nullptr))
        return fail(FIC_E_HIP, "fic_debug_qt_select_weighted: launch failed");
    if (e == hipSuccess) e = hipMemcpy(res, scratch + o_sel + 4 * 256 * 8, sizeof(res), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(FIC_E_HIP, "fic_debug_qt_select_weighted: %s", hipGetErrorString(e));
    *key_out = (uint32_t)res[0];
    *above_out = (int64_t)res[1];
    *gain_out = (int64_t)res[2];
    return FIC_OK;
}

}  // extern "C"
