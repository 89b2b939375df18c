// fic_capi_quadtree.cpp -- C ABI, quadtree (variable block size) codec, grey and joint RGB.  The encode is one pipeline with two
// front ends: qt_tree_run below -- collage SSE, the split rule's keys and select, compaction and statistics on the device
// (fic_quadtree.hip), every area where the plan of fic_qt_batch_plan.h puts it, every parameter read from device memory -- runs
// behind the level encodes of the one-shot entries here (qt_encode: idle-cached one-shot contexts, a plan of one plane, the null
// stream, results copied back at the end) and of the batched handle (fic_capi_qt_ctx.cpp).  Also here: the decoders of leaves of
// mixed size on the decode job (fic_internal.h).  The tag-2 (grey), tag-3 (colour) and tag-6 (colour with an isometry column)
// stream writers and parsers are in fic_stream.cpp.  Host-side orchestration only.  Semantics: DESIGN.md sections 4.13 (grey),
// 4.14 (colour), 4.17 (colour with the 8 isometries), 4.18 (encode to a leaf budget), 4.23 (pruning) and 4.24 (the pipeline).
#include "fic_internal.h"

using namespace ficd;

static_assert(kQtPlanSelectWords == FIC_QT_SELECT_WORDS && kQtPlanSelectWords == FIC_QT_SELECT_W_WORDS, "the plan's select areas");

namespace ficd {

template <typename Dev>
int qt_tree_run(const char* kind, const QtBatchPlan& Q, char* store, const QtLevels& L, const QtViews<typename Dev::Px>* views, QtRule rule,
                int goal, bool stats, hipStream_t s)
{
    auto at = [&](QtArea a) { return (void*)(store + Q.a[a].off); };
    const FicGeom& top = L.g[0];
    FicQtPlanes B{};
    B.planes = Q.planes;
    B.nkeys = Q.nkeys;
    B.sse_stride = Q.a[kQtSse].stride;
    B.leaf_stride = Q.a[kQtLeaves].stride;
    B.n_leaves = (int*)at(kQtNLeaves);
    B.param = (uint32_t*)at(kQtParam);
    B.ranks = (const uint32_t*)at(kQtRanks);
    B.values = (const long long*)at(kQtValues);
    const uint32_t* sse[kQtMaxLevels];
    const int32_t* qrows[kQtMaxLevels];
    const int32_t* iso[kQtMaxLevels];
    int Rw[kQtMaxLevels];
    for (int l = 0; l < L.nl; l++) {
        const auto& v = views[l];
        uint32_t* d_sse = (uint32_t*)at(kQtSse) + Q.sse_level[l];
        B.Nr[l] = L.g[l].Nr;
        Rw[l] = L.g[l].Rw;
        sse[l] = d_sse;
        qrows[l] = v.qrows;
        iso[l] = v.iso;
        if (fic_launch_leaf_sse<Dev>(v.image, v.scaled, v.qrows, v.iso, d_sse, L.g[l], s, B)) return fail(FIC_E_HIP, "k_leaf_sse launch failed");
    }
    uint32_t* d_keys = (uint32_t*)at(kQtKeys);
    if (rule == kRuleBudget) {            // the threshold's bits to param
        if (fic_launch_qt_keys(sse, Rw, L.nl, top.B, top.Rw, top.Nr, Q.n1, d_keys, s, B) ||
            fic_launch_qt_select(d_keys, (uint32_t)Q.nkeys, (uint32_t*)at(kQtSelect), s, B, 1))
            return fail(FIC_E_HIP, "%s budget select launch failed", kind);
    } else if (rule == kRuleRd) {         // lambda to param, unless it is there already (FIC_QT_RD_LAMBDA)
        long long* d_gains = (long long*)at(kQtGains);
        unsigned long long* d_top = (unsigned long long*)at(kQtTopSum);
        if (fic_launch_qt_rd_keys(sse, Rw, L.nl, top.B, top.Rw, top.Nr, Q.n1, d_keys, d_gains, d_top, s, B))
            return fail(FIC_E_HIP, "%s pruning keys launch failed", kind);
        int bad = 0;
        if (goal == FIC_QT_RD_LEAVES) bad = fic_launch_qt_select(d_keys, (uint32_t)Q.nkeys, (uint32_t*)at(kQtSelect), s, B, 0);
        else if (goal == FIC_QT_RD_SSE) bad = fic_launch_qt_select_w(d_keys, d_gains, (uint32_t)Q.nkeys, d_top, (unsigned long long*)at(kQtSelect), s, B);
        if (bad) return fail(FIC_E_HIP, "%s pruning select launch failed", kind);
    }
    int *d_cnt = (int*)at(kQtCounts), *d_offs = (int*)at(kQtOffs);
    int32_t* d_leaves = (int32_t*)at(kQtLeaves);
    unsigned long long* d_stats = (unsigned long long*)at(kQtStats);
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "stats4");
    if (rule == kRuleRd ? fic_launch_qt_compact_rd<Dev>(sse, qrows, iso, Rw, L.nl, top.B, top.Rw, top.Nr, d_keys, B.param, d_cnt, d_offs, d_leaves, s, B)
                        : fic_launch_qt_compact<Dev>(sse, qrows, iso, Rw, L.nl, top.B, top.Rw, top.Nr, d_cnt, d_offs, d_leaves, s, B))
        return fail(FIC_E_HIP, "%s compaction launch failed", kind);
    if (stats && (rule == kRuleRd ? fic_launch_qt_tree_stats_rd(sse, Rw, L.nl, top.B, top.Rw, top.Nr, d_keys, B.param, d_stats, s, B)
                                  : fic_launch_qt_tree_stats(sse, Rw, L.nl, top.B, top.Rw, top.Nr, d_stats, s, B)))
        return fail(FIC_E_HIP, "%s tree statistics launch failed", kind);
    return FIC_OK;
}
template int qt_tree_run<QtGrey>(const char*, const QtBatchPlan&, char*, const QtLevels&, const QtViews<uint8_t>*, QtRule, int, bool, hipStream_t);
template int qt_tree_run<QtRgb>(const char*, const QtBatchPlan&, char*, const QtLevels&, const QtViews<int32_t>*, QtRule, int, bool, hipStream_t);
template int qt_tree_run<QtRgbIso>(const char*, const QtBatchPlan&, char*, const QtLevels&, const QtViews<int32_t>*, QtRule, int, bool, hipStream_t);

}  // namespace ficd

namespace {

// ---- the host side of a pixel format (QtGrey / QtRgb / QtRgbIso, fic_launch.h) --------------------------------------------
// The one-shot contexts an encode runs its levels through, their device buffers and the stream format (fic_stream.h).
struct QtGreyHost : QtGrey {
    using Dev = QtGrey;               // the tag of the launchers
    using Ctx = fic_ctx;
    static constexpr const QtFormat& kStream = kQtGreyStream;
    static constexpr const DecodeKind& kDecode = kDecodeGrey;
    static int encode(Ctx* c, const uint8_t* gray, const int32_t* argb)   // exactly the one-shot encode of this level
    {
        const int rc = gray ? fic_ctx_set_gray_host(c, gray) : fic_ctx_set_argb_host(c, argb);
        return rc ? rc : fic_ctx_encode(c, 0, -1, nullptr);
    }
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
    static int encode(Ctx* c, const uint8_t*, const int32_t* argb)   // exactly the one-shot RGB encode of this level (n_iso = 1)
    {
        const int rc = fic_rgb_ctx_set_argb_host(c, argb);
        return rc ? rc : fic_rgb_ctx_encode(c, 0, nullptr);
    }
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
    static int encode(Ctx* c, const uint8_t* gray, const int32_t* argb) { return QtRgbHost::encode(c, gray, argb); }   // = fic_encode_rgb_iso_argb's / _lsq_argb's
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
    int Nr[kQtMaxLevels] = {0, 0, 0};
    for (int l = 0; l < L.nl; l++) Nr[l] = L.g[l].Nr;
    QtBatchPlan Q;                   // one plane: takes every image qt_levels takes (tests/cpp/qt_oneshot_plan_test.cpp)
    const char* why = "";
    if (qt_batch_plan(1, L.nl, Nr, Fmt::kLeafInts, &Q, &why))
        return fail(FIC_E_GEOMETRY, "%s encode: %dx%d, %d -> %d: %s would pass 2^31 - 1", Fmt::kStream.kind, w, h, B_max, B_min, why);
    const size_t sse_total = Q.a[kQtSse].stride;
    if (sse_out && sse_capacity < (int64_t)sse_total)
        return fail(FIC_E_CAPACITY, "%s SSE: need %zu values, have %lld", Fmt::kStream.kind, sse_total, (long long)sse_capacity);
    rc = check_device(device);
    if (rc) return rc;

    // one lease per level, under `search` for the call (least squares: DESIGN.md 4.19 / 4.20): parked again after success only
    Lease<typename Fmt::Ctx> lease[kQtMaxLevels];
    typename Fmt::Ctx* c[kQtMaxLevels] = {nullptr, nullptr, nullptr};
    DevMem mem(device);              // the store of this call: freed on every way out
    char* store = nullptr;
    for (int l = 0; l < L.nl && rc == FIC_OK; l++) {
        const FicGeom& g = L.g[l];
        rc = lease[l].open(device, g.W, g.H, g.B, g.wK, g.n_iso, search);
        c[l] = lease[l].c;
        if (rc == FIC_OK) rc = Fmt::encode(c[l], gray, argb);
    }
    if (rc == FIC_OK) rc = mem.alloc(store, Q.total);
    if (rc == FIC_OK && Fmt::prepare(c[0])) rc = fail(FIC_E_HIP, "k_scale launch failed");
    // the rule's parameter into the store, where the kernels read it: the threshold's bits or a given lambda, the rank of a leaf
    // budget, or the summed gain an SSE target asks for (sum S_top - max_sse; the sum is the device's)
    QtArea up = kQtParam;
    uint64_t word = 0;
    if (budget || (rd && rd->goal == FIC_QT_RD_LEAVES)) {
        up = kQtRanks;
        word = qt_rank(budget ? (uint64_t)budget->max_leaves : rd->value, Q);
    } else if (rd && rd->goal == FIC_QT_RD_SSE) {
        up = kQtValues;
        word = rd->value < (uint64_t)INT64_MAX ? rd->value : (uint64_t)INT64_MAX;
    } else if (rd) {
        word = (uint32_t)rd->value;
    } else {
        uint32_t bits;
        memcpy(&bits, &threshold, sizeof(bits));
        word = bits;
    }
    for (size_t i = 0; i < Q.a[up].elem / 4 && rc == FIC_OK; i++) {
        hipError_t e = hipMemsetD32Async((hipDeviceptr_t)(store + Q.a[up].off + 4 * i), (int)(uint32_t)(word >> (32 * i)), 1, nullptr);
        if (e != hipSuccess) rc = fail(FIC_E_HIP, "%s encode: %s", Fmt::kStream.kind, hipGetErrorString(e));
    }
    uint64_t* stats4 = budget ? budget->stats4 : (rd ? rd->stats4 : nullptr);
    if (rc == FIC_OK) {
        QtViews<typename Fmt::Px> views[kQtMaxLevels];
        for (int l = 0; l < L.nl; l++) views[l] = Fmt::views(c[l], c[0]);
        rc = qt_tree_run<typename Fmt::Dev>(Fmt::kStream.kind, Q, store, L, views, rd ? kRuleRd : (budget ? kRuleBudget : kRuleThreshold), rd ? rd->goal : 0,
                                            stats4 != nullptr, nullptr);
    }
    // Everything is enqueued; what the caller asked for comes back now.  n_leaves, param and stats are neighbours in the store.
    int n = 0;
    if (rc == FIC_OK) {
        const size_t first = Q.a[kQtNLeaves].off;
        std::vector<char> res(Q.a[kQtStats].off + 4 * sizeof(uint64_t) - first);
        const char *param = res.data() + (Q.a[kQtParam].off - first), *stats = res.data() + (Q.a[kQtStats].off - first);
        hipError_t e = hipMemcpy(res.data(), store + first, res.size(), hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(FIC_E_HIP, "%s encode: %s", Fmt::kStream.kind, hipGetErrorString(e));
        else {
            memcpy(&n, res.data(), sizeof(n));
            if (n_leaves) *n_leaves = n;
            if (budget) memcpy(budget->threshold_out, param, sizeof(float));
            if (rd) memcpy(rd->lambda_out, param, sizeof(uint32_t));
            if (stats4) memcpy(stats4, stats, 4 * sizeof(uint64_t));
        }
    }
    if (rc == FIC_OK && leaves) {
        if (capacity < n) rc = fail(FIC_E_CAPACITY, "%s encode: %d leaves, room for %lld", Fmt::kStream.kind, n, (long long)capacity);
        else {
            hipError_t e = hipMemcpy(leaves, store + Q.a[kQtLeaves].off, (size_t)n * Fmt::kLeafInts * 4, hipMemcpyDeviceToHost);
            if (e != hipSuccess) rc = fail(FIC_E_HIP, "%s encode: %s", Fmt::kStream.kind, hipGetErrorString(e));
        }
    }
    if (rc == FIC_OK && sse_out) {   // the levels of a plane lie one behind the other, as the caller gets them
        hipError_t e = hipMemcpy(sse_out, store + Q.a[kQtSse].off, sse_total * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(FIC_E_HIP, "%s SSE: %s", Fmt::kStream.kind, hipGetErrorString(e));
    }
    for (Lease<typename Fmt::Ctx>& l : lease) l.close(rc);
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
    // the keys, the select's area, then the one plane's rank and parameter word
    const size_t keys_bytes = align256((size_t)n * 4);
    rc = mem.alloc(scratch, keys_bytes + (FIC_QT_SELECT_WORDS + 2) * 4);
    if (rc) return rc;
    uint32_t *d_work = (uint32_t*)(scratch + keys_bytes), *d_rank = d_work + FIC_QT_SELECT_WORDS;
    FicQtPlanes P{};
    P.planes = 1;
    P.ranks = d_rank;
    P.param = d_rank + 1;
    const uint32_t r = (uint32_t)(rank < n ? rank : n);
    uint32_t res[4] = {0, 0, 0, 0};
    hipError_t e = hipMemcpy(scratch, keys, (size_t)n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_rank, &r, sizeof(r), hipMemcpyHostToDevice);
    if (e == hipSuccess && fic_launch_qt_select((const uint32_t*)scratch, (uint32_t)n, d_work, nullptr, P, 1))
        return fail(FIC_E_HIP, "fic_debug_qt_select: launch failed");
    if (e == hipSuccess) e = hipMemcpy(res, d_work + 4 * 256, sizeof(res), hipMemcpyDeviceToHost);
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
    size_t sum = 0;                     // the SSE of all levels, concatenated like the caller's: one copy
    for (int B = B_max; B >= B_min; B /= 2, nl++) {
        Rw[nl] = w / B;
        Nr[nl] = (w / B) * (h / B);
        sum += (size_t)Nr[nl];
    }
    const int n1 = nl == 3 ? Nr[1] : 0, nkeys = Nr[0] + n1;
    const size_t o_keys = align256(sum * 4), o_gains = o_keys + align256((size_t)nkeys * 4), o_top = o_gains + align256((size_t)nkeys * 8);
    DevMem mem(device);
    char* scratch = nullptr;
    rc = mem.alloc(scratch, o_top + 256);
    if (rc) return rc;
    const uint32_t* lv[kQtMaxLevels] = {nullptr, nullptr, nullptr};
    FicQtPlanes P{};                    // one plane of these levels; the key kernel takes no parameter
    P.planes = 1;
    P.nkeys = nkeys;
    P.sse_stride = sum;
    for (int l = 0; l < nl; l++) {
        lv[l] = l ? lv[l - 1] + Nr[l - 1] : (const uint32_t*)scratch;
        P.Nr[l] = Nr[l];
    }
    hipError_t e = hipMemcpy(scratch, sse, sum * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && fic_launch_qt_rd_keys(lv, Rw, nl, B_max, Rw[0], Nr[0], n1, (uint32_t*)(scratch + o_keys), (long long*)(scratch + o_gains),
                                                 (unsigned long long*)(scratch + o_top), nullptr, P))
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
    // the keys, the gains, the select's area, then the one plane's {total, value} = {need, 0} and its parameter word
    const size_t o_gains = align256((size_t)n * 4), o_work = o_gains + align256((size_t)n * 8);
    rc = mem.alloc(scratch, o_work + (FIC_QT_SELECT_W_WORDS + 3) * 8);
    if (rc) return rc;
    unsigned long long *d_work = (unsigned long long*)(scratch + o_work), *d_need = d_work + FIC_QT_SELECT_W_WORDS;
    FicQtPlanes P{};
    P.planes = 1;
    P.values = (const long long*)d_need + 1;
    P.param = (uint32_t*)(d_need + 2);
    const int64_t tv[2] = {need, 0};
    uint64_t res[4] = {0, 0, 0, 0};
    hipError_t e = hipMemcpy(scratch, keys, (size_t)n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(scratch + o_gains, gains, (size_t)n * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_need, tv, sizeof(tv), hipMemcpyHostToDevice);
    if (e == hipSuccess && fic_launch_qt_select_w((const uint32_t*)scratch, (const long long*)(scratch + o_gains), (uint32_t)n, d_need, d_work, nullptr, P))
        return fail(FIC_E_HIP, "fic_debug_qt_select_weighted: launch failed");
    if (e == hipSuccess) e = hipMemcpy(res, d_work + 4 * 256, sizeof(res), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(FIC_E_HIP, "fic_debug_qt_select_weighted: %s", hipGetErrorString(e));
    *key_out = (uint32_t)res[0];
    *above_out = (int64_t)res[1];
    *gain_out = (int64_t)res[2];
    return FIC_OK;
}

}  // extern "C"
