// fic_capi_lsq.cpp -- C ABI of the least-squares domain search: the winners' errors of a context and
// the one-shot entries, which are the reference's one-shot encode (encode_oneshot, fic_capi.cpp) on a lease under "search" = 1.
// The search itself is the option "search" = 1 of a context (fic_capi.cpp, kernels in fic_lsq.hip); the quadtree entries are in
// fic_capi_quadtree.cpp.  Host-side orchestration only.
#include "fic_internal.h"

using namespace ficd;

extern "C" {

int fic_ctx_get_lsq_error_host(fic_ctx* c, int64_t* E)
{
    if (!c || !E) return fail(FIC_E_ARGUMENT, "fic_ctx_get_lsq_error_host: null argument");
    return ctx_get_lsq_error(c, "fic_ctx_get_lsq_error_host", E);
}

int fic_encode_gray_lsq_u8(const uint8_t* gray, int w, int h, int B, int wK, int n_iso, int device, int32_t* idx_local, float* a,
                           float* b, int32_t* iso, int32_t* qrows, int64_t* E)
{
    return encode_oneshot(gray, nullptr, w, h, B, wK, n_iso, device, idx_local, a, b, iso, qrows, E, 1);
}

int fic_encode_gray_lsq_argb(const int32_t* argb, int w, int h, int B, int wK, int n_iso, int device, int32_t* idx_local, float* a,
                             float* b, int32_t* iso, int32_t* qrows, int64_t* E)
{
    return encode_oneshot(nullptr, argb, w, h, B, wK, n_iso, device, idx_local, a, b, iso, qrows, E, 1);
}

}  // extern "C"
