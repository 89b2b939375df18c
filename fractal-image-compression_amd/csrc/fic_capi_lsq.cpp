// fic_capi_lsq.cpp -- C ABI of the least-squares domain search: the winners' errors of a context and
// the one-shot entries over the cached contexts.  The search itself is the option "search" = 1 of a context (fic_capi.cpp,
// kernels in fic_lsq.hip); the quadtree entries are in fic_capi_quadtree.cpp.  Host-side orchestration only.
#include "fic_internal.h"

using namespace ficd;

namespace {

int lsq_oneshot(const uint8_t* gray, const int32_t* argb, int w, int h, int B, int wK, int n_iso, int device, int32_t* idx_local,
                float* a, float* b, int32_t* iso, int32_t* qrows, int64_t* E)
{
    if ((!gray && !argb) || !idx_local || !a || !b) return fail(FIC_E_ARGUMENT, "fic_encode_gray_lsq: null argument");
    fic_ctx* c = g_idle_grey.take(device, w, h, B, wK, n_iso);
    if (!c) c = fic_ctx_create(device, w, h, B, wK, n_iso, 1);
    if (!c) return g_err_code ? g_err_code : FIC_E_HIP;   // fic_ctx_create recorded why
    int rc = fic_ctx_set_option(c, "search", 1);
    if (rc == FIC_OK) rc = gray ? fic_ctx_set_gray_host(c, gray) : fic_ctx_set_argb_host(c, argb);
    if (rc == FIC_OK) rc = fic_ctx_encode(c, 0, -1, nullptr);
    if (rc == FIC_OK) rc = fic_ctx_get_results_host(c, idx_local, a, b, iso, qrows, nullptr, nullptr);
    if (rc == FIC_OK && E) rc = fic_ctx_get_lsq_error_host(c, E);
    ErrKeep keep;
    // the cached contexts serve the reference entries too: never parked in least-squares mode
    if (rc == FIC_OK && fic_ctx_set_option(c, "search", 0) == FIC_OK) g_idle_grey.give(c);
    else fic_ctx_destroy(c);
    return rc;
}

}  // namespace

extern "C" {

int fic_ctx_get_lsq_error_host(fic_ctx* c, int64_t* E)
{
    if (!c || !E) return fail(FIC_E_ARGUMENT, "fic_ctx_get_lsq_error_host: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->encoded_any || c->last_search != 1 || !c->lsq.E)
        return fail(FIC_E_STATE, "fic_ctx_get_lsq_error_host: the last encode was not a least-squares search (\"search\" = 1)");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->last_stream));
    static_assert(sizeof(long long) == sizeof(int64_t), "E");
    HIP_TRY(hipMemcpy(E, c->lsq.E, (size_t)c->g.planes * c->g.Nr * sizeof(int64_t), hipMemcpyDeviceToHost));
    return FIC_OK;
}

int fic_encode_gray_lsq_u8(const uint8_t* gray, int w, int h, int B, int wK, int n_iso, int device, int32_t* idx_local, float* a,
                           float* b, int32_t* iso, int32_t* qrows, int64_t* E)
{
    return lsq_oneshot(gray, nullptr, w, h, B, wK, n_iso, device, idx_local, a, b, iso, qrows, E);
}

int fic_encode_gray_lsq_argb(const int32_t* argb, int w, int h, int B, int wK, int n_iso, int device, int32_t* idx_local, float* a,
                             float* b, int32_t* iso, int32_t* qrows, int64_t* E)
{
    return lsq_oneshot(nullptr, argb, w, h, B, wK, n_iso, device, idx_local, a, b, iso, qrows, E);
}

}  // extern "C"
