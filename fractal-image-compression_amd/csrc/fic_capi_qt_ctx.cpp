// fic_capi_qt_ctx.cpp -- C ABI, the batched quadtree encoder handle (fic_qt_ctx_* of include/fic.h): `planes`
// images of one geometry through the per-level contexts (created with `planes`) and the batched kernels of fic_quadtree.hip,
// under the device-pointer contract and the stream rule of the other two handles.  An encode enqueues everything
// on the caller's stream and returns: the per-plane parameters go up from a pinned staging buffer, and nothing comes back before
// the caller asks.  This file is one of the two front ends of the one encode pipeline: what is its own is the input contract, the
// staging slots and the level encodes on contexts of `planes`; everything behind them is qt_tree_run (fic_capi_quadtree.cpp),
// which the one-shot entries of the same format run on a plan of one plane -- so plane p of a batch is what they return for
// image p.  Host-side orchestration only.
#include "fic_internal.h"

using namespace ficd;

// The levels are contexts of their own (grey: fic_ctx, colour: fic_rgb_ctx with the isometry column); `mem` owns the one device
// store (QtBatchPlan), the pinned staging buffer and a copy of a host input.
struct fic_qt_ctx : ficd::CtxCore {
    int colour = 0, B_max = 0, B_min = 0, n_iso = 1, planes = 1;
    QtLevels L;
    QtBatchPlan plan{};
    fic_ctx* grey[kQtMaxLevels] = {nullptr, nullptr, nullptr};
    fic_rgb_ctx* rgb[kQtMaxLevels] = {nullptr, nullptr, nullptr};
    char* store = nullptr;
    char* staging = nullptr;             // pinned: kQtPlanStagingSlots slots, each with the event of the copy that last read it
    hipEvent_t slot_ev[kQtPlanStagingSlots] = {};
    bool slot_busy[kQtPlanStagingSlots] = {};
    int next_slot = 0;
    uint8_t* gray_own = nullptr;         // a host input's device copy (grey), the staging of an ARGB upload to a grey context
    int32_t* argb_own = nullptr;
    char* dec_store = nullptr;           // decode and collage (QtDecodePlan, fic_qt_decode_plan.h): on first use
    template <typename T>
    T* at(QtArea a) const { return (T*)(store + plan.a[a].off); }
};

namespace {

const char* qt_kind(const fic_qt_ctx* c) { return c->colour ? kQtRgbIsoStream.kind : kQtGreyStream.kind; }

// every level gets the same device input (never copied)
int qt_ctx_input(fic_qt_ctx* c, const void* dev)
{
    for (int l = 0; l < c->L.nl; l++)
        if (int rc = c->colour ? fic_rgb_ctx_set_argb_device(c->rgb[l], dev) : fic_ctx_set_gray_device(c->grey[l], dev)) return rc;
    c->have_input = true;
    return FIC_OK;
}

// The common head of the three encodes: the state checks, the stream rule, a free staging slot.  Holds c->mu.
int qt_ctx_begin(fic_qt_ctx* c, const char* who, hipStream_t s, int* slot)
{
    if (!c->have_input) return fail(FIC_E_STATE, "%s: no input image set", who);
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = take_stream(c, s)) return rc;
    *slot = c->next_slot;
    if (c->slot_busy[*slot]) HIP_TRY(hipEventSynchronize(c->slot_ev[*slot]));      // the copy of four encodes ago: long done
    c->slot_busy[*slot] = false;
    return FIC_OK;
}

// Everything of an encode behind its checks, enqueued on s: the parameters' upload from staging slot `slot` (`up` says which
// area it fills) and the levels, then the shared pipeline on their device arrays.
template <typename Dev>
int qt_ctx_run(fic_qt_ctx* c, QtRule rule, int goal, QtArea up, int slot, hipStream_t s)
{
    const QtBatchPlan& Q = c->plan;
    const QtLevels& L = c->L;
    const size_t P = (size_t)c->planes;
    {
        const char* src = c->staging + (size_t)slot * Q.staging_slot + (up == kQtValues ? Q.staging_values : 0);
        HIP_TRY(hipMemcpyAsync(c->store + Q.a[up].off, src, P * Q.a[up].elem, hipMemcpyHostToDevice, s));
        HIP_TRY(hipEventRecord(c->slot_ev[slot], s));
        c->slot_busy[slot] = true;
        c->next_slot = (slot + 1) % kQtPlanStagingSlots;
    }
    for (int l = 0; l < L.nl; l++) {
        int rc = c->colour ? fic_rgb_ctx_set_option(c->rgb[l], "search", c->opt_search) : fic_ctx_set_option(c->grey[l], "search", c->opt_search);
        if (rc == FIC_OK) rc = c->colour ? fic_rgb_ctx_encode(c->rgb[l], 0, s) : fic_ctx_encode(c->grey[l], 0, -1, s);
        if (rc) return rc;
    }
    // grey: every level reads the top context's scaled copy, made here for all planes (the original, 2:1 scaled: FC:970-1007)
    if (!c->colour && fic_launch_scale(c->grey[0]->b.gray, c->grey[0]->b.scaled, c->grey[0]->g, s)) return fail(FIC_E_HIP, "k_scale launch failed");

    QtViews<typename Dev::Px> views[kQtMaxLevels];
    for (int l = 0; l < L.nl; l++) {
        if constexpr (sizeof(typename Dev::Px) == 1)
            views[l] = {c->grey[l]->b.gray, c->grey[0]->b.scaled, c->grey[l]->o.qrows, c->n_iso > 1 ? c->grey[l]->o.iso : nullptr};
        else    // every level reads its own scaleImageRGB copy, made by its encode; iso NULL on n_iso = 1: the identity
            views[l] = {c->rgb[l]->argb, c->rgb[l]->scaled, c->rgb[l]->qrows, c->rgb[l]->iso};
    }
    if (int rc = qt_tree_run<Dev>(qt_kind(c), Q, c->store, L, views, rule, goal, true, s)) return rc;
    c->encoded_any = true;
    return FIC_OK;
}

int qt_ctx_run_any(fic_qt_ctx* c, QtRule rule, int goal, QtArea up, int slot, hipStream_t s)
{
    return c->colour ? qt_ctx_run<QtRgbIso>(c, rule, goal, up, slot, s) : qt_ctx_run<QtGrey>(c, rule, goal, up, slot, s);
}

void qt_ctx_free(fic_qt_ctx* c)
{
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    for (hipEvent_t e : c->slot_ev)
        if (e) (void)hipEventDestroy(e);
    for (int l = 0; l < kQtMaxLevels; l++) {
        if (c->grey[l]) fic_ctx_destroy(c->grey[l]);
        if (c->rgb[l]) fic_rgb_ctx_destroy(c->rgb[l]);
    }
    delete c;
}

// ---- decode and collage of the last encode's tables ---------------------------------------------------------
// What both entries check and set up behind their null checks, holding c->mu: an encode has run, the levels at `zoom`
// (make_decode_geometry refuses another zoom and a side above 64), room in `out`, the decode store.  D: the kernels' view of
// the context; W: where the areas of the store lie.
int qt_ctx_decode_begin(fic_qt_ctx* c, const char* who, int zoom, int64_t capacity_pixels, FicQtDecode* D, QtDecodePlan* W)
{
    if (!c->encoded_any) return fail(FIC_E_STATE, "%s: nothing encoded yet", who);
    const QtLevels& L = c->L;
    const FicGeom& top = L.g[0];
    *D = FicQtDecode{};
    for (int l = 0; l < L.nl; l++)
        if (int rc = make_decode_geometry(top.W, top.H, L.g[l].B, L.g[l].wK, c->n_iso, c->planes, zoom, &D->g[l])) return rc;
    D->nl = L.nl;
    D->zoom = zoom;
    D->B_max = c->B_max;
    D->B_min = c->B_min;
    D->W = top.W;
    D->H = top.H;
    D->Rw_top = top.Rw;
    D->Rw_min = L.g[L.nl - 1].Rw;
    D->Nr_min = c->plan.Nr_min;
    D->n_iso = c->n_iso;
    D->leaf_stride = c->plan.a[kQtLeaves].stride;
    const size_t P = (size_t)c->planes, npix = (size_t)top.W * top.H;
    const char* why = "";
    if (qt_decode_plan(c->planes, top.W, top.H, c->B_min, c->colour ? 4 : 1, zoom, sizeof(FicDecodeState), fic_decode_sq_words(P, npix), W, &why))
        return fail(FIC_E_GEOMETRY, "%s: %d planes of %dx%d at zoom %d: %s would pass 2^31 - 1", who, c->planes, top.W, top.H, zoom, why);
    const long long need = (long long)P * D->g[0].W * D->g[0].H;
    if (capacity_pixels < need) return fail(FIC_E_CAPACITY, "%s: output needs %lld pixels, have %lld", who, need, (long long)capacity_pixels);
    HIP_TRY(hipSetDevice(c->device));
    return c->mem.ensure(c->dec_store, W->total);
}

// the decoder's message for a marked plane, under the entry's name
int qt_ctx_bad_table(const char* who, int rc)
{
    if (rc != FIC_E_ARGUMENT) return rc;
    return fail(FIC_E_ARGUMENT, "%s: the leaf table on the device is not a tiling this context's levels can decode (%s)", who, std::string(g_err).c_str());
}

template <typename Dev>
int qt_ctx_decode(fic_qt_ctx* c, const char* who, const FicQtDecode& D, const QtDecodePlan& W, void* out, float* avg_error_out, int* iterations_out)
{
    using Px = typename Dev::Px;
    const DecodeKind& kind = sizeof(Px) == 1 ? kDecodeGrey : kDecodeRgb;
    const FicGeom& g = D.g[0];                             // planes = the context's
    const hipStream_t s = c->last_stream;
    auto at = [&](QtDecodeArea a) { return (void*)(c->dec_store + W.a[a].off); };
    DecodeJob J;
    if (D.zoom != 1) {                                     // the store holds the encoded size: the loop's areas come from an arena
        if (int rc = J.open(who, c->device, kind, g, s)) return rc;
    } else {
        J.borrow(kind, g, s, at(kQtDecScaled), at(kQtDecImage), (FicDecodeState*)at(kQtDecState), (uint32_t*)at(kQtDecSq));
    }
    HIP_TRY(hipStreamSynchronize(s));
    int32_t *entries = (int32_t*)at(kQtDecEntries), *cells = (int32_t*)at(kQtDecCells), *cover = (int32_t*)at(kQtDecCover);
    // one iteration: before the first, the tables resolved (the loop has put its initial state on s by then); scale the
    // current image of every plane, one paint of all leaves of all planes, loop control
    const int rc = J.run(who, nullptr, avg_error_out, iterations_out, nullptr, out, [&](int counter) {
        if (counter == 0 && fic_launch_qt_resolve<Dev>(c->at<int32_t>(kQtLeaves), c->at<int>(kQtNLeaves), D, g.planes, entries, cells, cover, J.state, s))
            return -1;
        if constexpr (sizeof(Px) == 1) {
            if (fic_launch_scale((const uint8_t*)J.image, (uint8_t*)J.scaled, g, s)) return -1;
        } else {
            if (fic_launch_scale_rgb_planes((const int32_t*)J.image, (int32_t*)J.scaled, g, s)) return -1;
        }
        if (fic_launch_qt_paint_planes<Dev>((const Px*)J.scaled, (Px*)J.image, entries, cells, cover, J.state, J.sq, counter, false, D, g.planes, s))
            return -1;
        return fic_launch_decode_step(J.state, J.sq, counter, g.W * g.H, g.planes, s);
    });
    return qt_ctx_bad_table(who, rc);
}

template <typename Dev>
int qt_ctx_collage(fic_qt_ctx* c, const char* who, const FicQtDecode& D, const QtDecodePlan& W, void* out)
{
    using Px = typename Dev::Px;
    const FicGeom& g = D.g[0];
    const size_t P = (size_t)g.planes, npix = (size_t)g.W * g.H;
    const hipStream_t s = c->last_stream;
    auto at = [&](QtDecodeArea a) { return (void*)(c->dec_store + W.a[a].off); };
    FicDecodeState* d_state = (FicDecodeState*)at(kQtDecState);
    int32_t *entries = (int32_t*)at(kQtDecEntries), *cells = (int32_t*)at(kQtDecCells), *cover = (int32_t*)at(kQtDecCover);
    // the 2:1 copy of the input the level encodes made: the top grey context's for every level, the top colour context's own
    const Px* scaled;
    if constexpr (sizeof(Px) == 1) scaled = c->grey[0]->b.scaled;
    else scaled = c->rgb[0]->scaled;
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipMemsetAsync(d_state, 0, P * sizeof(FicDecodeState), s));
    if (fic_launch_qt_resolve<Dev>(c->at<int32_t>(kQtLeaves), c->at<int>(kQtNLeaves), D, g.planes, entries, cells, cover, d_state, s) ||
        fic_launch_qt_paint_planes<Dev>(scaled, (Px*)at(kQtDecImage), entries, cells, cover, d_state, nullptr, 0, true, D, g.planes, s))
        return fail(FIC_E_HIP, "%s: launch failed", who);
    std::vector<FicDecodeState> st(P);
    HIP_TRY(hipMemcpyAsync(st.data(), d_state, P * sizeof(FicDecodeState), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (size_t p = 0; p < P; p++)
        if (st[p].bad_index)
            return fail(FIC_E_ARGUMENT, "%s: the leaf table of plane %zu on the device is not a tiling this context's levels can decode", who, p);
    HIP_TRY(hipMemcpy(out, at(kQtDecImage), P * npix * sizeof(Px), hipMemcpyDeviceToHost));
    return FIC_OK;
}

}  // namespace

extern "C" {

fic_qt_ctx* fic_qt_ctx_create(int device, int colour, int w, int h, int B_max, int B_min, int wK, int n_iso, int planes)
{
    if (colour != 0 && colour != 1) { fail(FIC_E_ARGUMENT, "fic_qt_ctx_create: colour = %d, need 0 (grey) or 1 (joint RGB)", colour); return nullptr; }
    QtLevels L;
    if (qt_levels(w, h, B_max, B_min, wK, n_iso, &L)) return nullptr;
    if (planes < 1) { fail(FIC_E_ARGUMENT, "planes=%d", planes); return nullptr; }
    int Nr[kQtMaxLevels] = {0, 0, 0};
    for (int l = 0; l < L.nl; l++) Nr[l] = L.g[l].Nr;
    QtBatchPlan plan;
    const char* why = "";
    if (qt_batch_plan(planes, L.nl, Nr, colour ? QtRgbIso::kLeafInts : QtGrey::kLeafInts, &plan, &why)) {
        fail(FIC_E_GEOMETRY, "fic_qt_ctx_create: %d planes of %dx%d, %d -> %d: %s would pass 2^31 - 1", planes, w, h, B_max, B_min, why);
        return nullptr;
    }
    if (!create_device_ok(device)) return nullptr;
    fic_qt_ctx* c = new fic_qt_ctx();
    c->device = device;
    c->mem.set_device(device);
    c->colour = colour;
    c->B_max = B_max;
    c->B_min = B_min;
    c->n_iso = n_iso;
    c->planes = planes;
    c->L = L;
    c->g = L.g[0];
    c->g.planes = planes;
    c->plan = plan;
    int rc = FIC_OK;
    for (int l = 0; l < L.nl && rc == FIC_OK; l++) {
        const FicGeom& g = L.g[l];
        if (colour) c->rgb[l] = fic_rgb_ctx_create_iso(device, w, h, g.B, g.wK, n_iso, planes);
        else c->grey[l] = fic_ctx_create(device, w, h, g.B, g.wK, n_iso, planes);
        if (!c->rgb[l] && !c->grey[l]) rc = g_err_code ? g_err_code : FIC_E_HIP;
    }
    if (rc == FIC_OK) rc = c->mem.alloc(c->store, plan.total);
    if (rc == FIC_OK) rc = c->mem.alloc(c->staging, plan.staging_slot * kQtPlanStagingSlots, kMemPinned);
    for (int i = 0; i < kQtPlanStagingSlots && rc == FIC_OK; i++)
        if (hipEventCreateWithFlags(&c->slot_ev[i], hipEventDisableTiming) != hipSuccess) rc = fail(FIC_E_HIP, "fic_qt_ctx_create: hipEventCreateWithFlags failed");
    if (rc == FIC_OK) {
        // results read before the first encode are zeros.  The fill is only enqueued (null stream); encodes run on other streams
        hipError_t e = hipMemset(c->store, 0, plan.total);
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        if (e != hipSuccess) rc = fail(FIC_E_HIP, "fic_qt_ctx_create: hipMemset: %s", hipGetErrorString(e));
    }
    if (rc != FIC_OK) {
        ErrKeep keep;
        qt_ctx_free(c);
        return nullptr;
    }
    return c;
}

void fic_qt_ctx_destroy(fic_qt_ctx* c)
{
    if (c) qt_ctx_free(c);
}

int fic_qt_ctx_set_gray_host(fic_qt_ctx* c, const uint8_t* gray)
{
    if (!c || !gray) return fail(FIC_E_ARGUMENT, "fic_qt_ctx_set_gray_host: null argument");
    if (c->colour) return fail(FIC_E_ARGUMENT, "fic_qt_ctx_set_gray_host: a colour context takes ARGB input");
    std::lock_guard<std::mutex> lk(c->mu);
    if (int rc = upload_input(c, c->gray_own, gray, (size_t)c->planes * c->g.W * c->g.H)) return rc;
    return qt_ctx_input(c, c->gray_own);
}

int fic_qt_ctx_set_argb_host(fic_qt_ctx* c, const int32_t* argb)
{
    if (!c || !argb) return fail(FIC_E_ARGUMENT, "fic_qt_ctx_set_argb_host: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    const size_t npix = (size_t)c->planes * c->g.W * c->g.H;
    if (int rc = c->colour ? upload_input(c, c->argb_own, argb, npix) : upload_argb_as_gray(c, c->argb_own, c->gray_own, argb, npix)) return rc;
    return qt_ctx_input(c, c->colour ? (const void*)c->argb_own : (const void*)c->gray_own);
}

int fic_qt_ctx_set_gray_device(fic_qt_ctx* c, const void* dev_gray)
{
    if (!c || !dev_gray) return fail(FIC_E_ARGUMENT, "fic_qt_ctx_set_gray_device: null argument");
    if (c->colour) return fail(FIC_E_ARGUMENT, "fic_qt_ctx_set_gray_device: a colour context takes ARGB input");
    // fic_ctx_set_gray_device's rule, refused here before any level has taken the pointer
    if (int rc = check_input_alignment("fic_qt_ctx_set_gray_device", dev_gray, 8)) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    return qt_ctx_input(c, dev_gray);
}

int fic_qt_ctx_set_argb_device(fic_qt_ctx* c, const void* dev_argb)
{
    if (!c || !dev_argb) return fail(FIC_E_ARGUMENT, "fic_qt_ctx_set_argb_device: null argument");
    if (!c->colour) return fail(FIC_E_ARGUMENT, "fic_qt_ctx_set_argb_device: a grey context takes device input as bytes (fic_qt_ctx_set_gray_device)");
    if (int rc = check_input_alignment("fic_qt_ctx_set_argb_device", dev_argb, 4)) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    return qt_ctx_input(c, dev_argb);
}

int fic_qt_ctx_set_option(fic_qt_ctx* c, const char* name, int value)
{
    if (!c || !name) return fail(FIC_E_ARGUMENT, "fic_qt_ctx_set_option: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    return set_core_option(c, kOptQt, "fic_qt_ctx_set_option: ", name, value);     // "search": the levels get it at encode time
}

int fic_qt_ctx_encode_threshold(fic_qt_ctx* c, const float* thresholds, void* hip_stream)
{
    if (!c || !thresholds) return fail(FIC_E_ARGUMENT, "fic_qt_ctx_encode_threshold: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    for (int p = 0; p < c->planes; p++)
        if (thresholds[p] != thresholds[p]) return fail(FIC_E_ARGUMENT, "%s encode: threshold is NaN (plane %d)", qt_kind(c), p);
    int slot = 0;
    hipStream_t s = (hipStream_t)hip_stream;
    if (int rc = qt_ctx_begin(c, "fic_qt_ctx_encode_threshold", s, &slot)) return rc;
    memcpy(c->staging + (size_t)slot * c->plan.staging_slot, thresholds, (size_t)c->planes * sizeof(float));
    return qt_ctx_run_any(c, kRuleThreshold, 0, kQtParam, slot, s);
}

int fic_qt_ctx_encode_budget(fic_qt_ctx* c, const int64_t* max_leaves, void* hip_stream)
{
    if (!c || !max_leaves) return fail(FIC_E_ARGUMENT, "fic_qt_ctx_encode_budget: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->opt_search != 0)
        return fail(FIC_E_ARGUMENT, "fic_qt_ctx_encode_budget: the threshold budget runs on the reference's criterion only (\"search\" = 0); fic_qt_ctx_encode_rd takes both");
    const FicGeom& top = c->L.g[0];
    for (int p = 0; p < c->planes; p++)
        if (max_leaves[p] < top.Nr)
            return fail(FIC_E_ARGUMENT, "%s encode: max_leaves = %lld, the image has %d blocks of side %d (plane %d)", qt_kind(c), (long long)max_leaves[p],
                        top.Nr, top.B, p);
    int slot = 0;
    hipStream_t s = (hipStream_t)hip_stream;
    if (int rc = qt_ctx_begin(c, "fic_qt_ctx_encode_budget", s, &slot)) return rc;
    uint32_t* ranks = (uint32_t*)(c->staging + (size_t)slot * c->plan.staging_slot);
    for (int p = 0; p < c->planes; p++) ranks[p] = qt_rank((uint64_t)max_leaves[p], c->plan);
    return qt_ctx_run_any(c, kRuleBudget, 0, kQtRanks, slot, s);
}

int fic_qt_ctx_encode_rd(fic_qt_ctx* c, int goal, const uint64_t* values, void* hip_stream)
{
    const char* entry = "fic_qt_ctx_encode_rd";
    if (!c || !values) return fail(FIC_E_ARGUMENT, "%s: null argument", entry);
    if (goal < FIC_QT_RD_LAMBDA || goal > FIC_QT_RD_SSE) return fail(FIC_E_ARGUMENT, "%s: goal = %d, need 0 (lambda), 1 (leaves) or 2 (SSE)", entry, goal);
    std::lock_guard<std::mutex> lk(c->mu);
    const FicGeom& top = c->L.g[0];
    for (int p = 0; p < c->planes; p++) {
        if (goal == FIC_QT_RD_LAMBDA && values[p] > 0xFFFFFFFFull)
            return fail(FIC_E_ARGUMENT, "%s: lambda = %llu, need 0 .. 2^32 - 1 (plane %d)", entry, (unsigned long long)values[p], p);
        if (goal == FIC_QT_RD_LEAVES && values[p] < (uint64_t)top.Nr)
            return fail(FIC_E_ARGUMENT, "%s encode: max_leaves = %llu, the image has %d blocks of side %d (plane %d)", qt_kind(c),
                        (unsigned long long)values[p], top.Nr, top.B, p);
    }
    int slot = 0;
    hipStream_t s = (hipStream_t)hip_stream;
    if (int rc = qt_ctx_begin(c, entry, s, &slot)) return rc;
    char* stage = c->staging + (size_t)slot * c->plan.staging_slot;
    QtArea up = kQtParam;
    if (goal == FIC_QT_RD_LAMBDA) {
        for (int p = 0; p < c->planes; p++) ((uint32_t*)stage)[p] = (uint32_t)values[p];
    } else if (goal == FIC_QT_RD_LEAVES) {
        up = kQtRanks;
        for (int p = 0; p < c->planes; p++) ((uint32_t*)stage)[p] = qt_rank(values[p], c->plan);
    } else {                                           // the summed gain has to reach sum S_top - max_sse
        up = kQtValues;
        const uint64_t cap = (uint64_t)INT64_MAX;
        for (int p = 0; p < c->planes; p++) ((long long*)(stage + c->plan.staging_values))[p] = (long long)(values[p] < cap ? values[p] : cap);
    }
    return qt_ctx_run_any(c, kRuleRd, goal, up, slot, s);
}

int fic_qt_ctx_sync(fic_qt_ctx* c)
{
    if (!c) return fail(FIC_E_ARGUMENT, "fic_qt_ctx_sync: null context");
    std::lock_guard<std::mutex> lk(c->mu);
    if (int rc = ctx_sync(c)) return rc;
    // the levels ran on the same stream: nothing of theirs is pending either, and none waits for that stream again
    for (int l = 0; l < c->L.nl; l++)
        if (int rc = c->colour ? fic_rgb_ctx_sync(c->rgb[l]) : fic_ctx_sync(c->grey[l])) return rc;
    return FIC_OK;
}

int fic_qt_ctx_get_results_host(fic_qt_ctx* c, int32_t* n_leaves, uint32_t* param, uint64_t* stats)
{
    if (!c) return fail(FIC_E_ARGUMENT, "fic_qt_ctx_get_results_host: null context");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->encoded_any) return fail(FIC_E_STATE, "fic_qt_ctx_get_results_host: nothing encoded yet");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->last_stream));
    // the three areas follow each other in the store: one copy
    const QtBatchPlan& Q = c->plan;
    const size_t P = (size_t)c->planes, o0 = Q.a[kQtNLeaves].off, bytes = Q.a[kQtStats].off + P * 32 - o0;
    std::vector<char> buf(bytes);
    HIP_TRY(hipMemcpy(buf.data(), c->store + o0, bytes, hipMemcpyDeviceToHost));
    if (n_leaves) memcpy(n_leaves, buf.data(), P * 4);
    if (param) memcpy(param, buf.data() + (Q.a[kQtParam].off - o0), P * 4);
    if (stats) memcpy(stats, buf.data() + (Q.a[kQtStats].off - o0), P * 32);
    return FIC_OK;
}

int fic_qt_ctx_get_leaves_host(fic_qt_ctx* c, int plane, int32_t* leaves, int64_t capacity, int* n_leaves)
{
    if (!c || !leaves || !n_leaves) return fail(FIC_E_ARGUMENT, "fic_qt_ctx_get_leaves_host: null argument");
    if (plane < 0 || plane >= c->planes) return fail(FIC_E_ARGUMENT, "fic_qt_ctx_get_leaves_host: plane %d outside 0..%d", plane, c->planes - 1);
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->encoded_any) return fail(FIC_E_STATE, "fic_qt_ctx_get_leaves_host: nothing encoded yet");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->last_stream));
    int n = 0;
    HIP_TRY(hipMemcpy(&n, c->at<int>(kQtNLeaves) + plane, sizeof(int), hipMemcpyDeviceToHost));
    *n_leaves = n;
    if (capacity < n) return fail(FIC_E_CAPACITY, "%s encode: %d leaves, room for %lld", qt_kind(c), n, (long long)capacity);
    const size_t stride = c->plan.a[kQtLeaves].stride;
    HIP_TRY(hipMemcpy(leaves, c->at<int32_t>(kQtLeaves) + (size_t)plane * stride, (size_t)n * c->plan.leaf_ints * 4, hipMemcpyDeviceToHost));
    return FIC_OK;
}

int fic_qt_ctx_result_device_ptrs(fic_qt_ctx* c, void** leaves, void** n_leaves, void** param, void** stats)
{
    if (!c) return fail(FIC_E_ARGUMENT, "fic_qt_ctx_result_device_ptrs: null context");
    if (leaves) *leaves = c->at<void>(kQtLeaves);
    if (n_leaves) *n_leaves = c->at<void>(kQtNLeaves);
    if (param) *param = c->at<void>(kQtParam);
    if (stats) *stats = c->at<void>(kQtStats);
    return FIC_OK;
}

int fic_qt_ctx_decode_zoom_host(fic_qt_ctx* c, int zoom, void* out, int64_t capacity_pixels, float* avg_error_out, int* iterations_out)
{
    const char* who = "fic_qt_ctx_decode_zoom_host";
    if (!c || !out) return fail(FIC_E_ARGUMENT, "%s: null argument", who);
    std::lock_guard<std::mutex> lk(c->mu);
    FicQtDecode D;
    QtDecodePlan W;
    if (int rc = qt_ctx_decode_begin(c, who, zoom, capacity_pixels, &D, &W)) return rc;
    return c->colour ? qt_ctx_decode<QtRgbIso>(c, who, D, W, out, avg_error_out, iterations_out)
                     : qt_ctx_decode<QtGrey>(c, who, D, W, out, avg_error_out, iterations_out);
}

int fic_qt_ctx_collage_host(fic_qt_ctx* c, void* out, int64_t capacity_pixels)
{
    const char* who = "fic_qt_ctx_collage_host";
    if (!c || !out) return fail(FIC_E_ARGUMENT, "%s: null argument", who);
    std::lock_guard<std::mutex> lk(c->mu);
    FicQtDecode D;
    QtDecodePlan W;
    if (int rc = qt_ctx_decode_begin(c, who, 1, capacity_pixels, &D, &W)) return rc;
    return c->colour ? qt_ctx_collage<QtRgbIso>(c, who, D, W, out) : qt_ctx_collage<QtGrey>(c, who, D, W, out);
}

}  // extern "C"
