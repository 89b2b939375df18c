// fic_ctx_core.cpp -- what fic_ctx, fic_rgb_ctx and fic_qt_ctx do alike, over the core they share (ficd::CtxCore,
// fic_internal.h), once: the stream rule, the sweep timer, the growth of the least-squares slot stores, the read-out of a debug
// store, the sync entry, the shared options (their rules: fic_ctx_options.h) with the "sweep_stats" counter block, the getters
// that differ only in the handle type, and the upload of a host input.  Host-side orchestration only.
#include "fic_internal.h"

namespace ficd {

CtxCore::~CtxCore()
{
    if (timer.ev.empty()) return;
    (void)hipSetDevice(device);
    for (hipEvent_t e : timer.ev) (void)hipEventDestroy(e);
}

int take_stream(CtxCore* c, hipStream_t s)
{
    if (s != c->last_stream) {
        if (c->stream_used) HIP_TRY(hipStreamSynchronize(c->last_stream));
        c->last_stream = s;
    }
    c->stream_used = true;
    return FIC_OK;
}

int ctx_sync(CtxCore* c)
{
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->last_stream));
    c->stream_used = false;                             // nothing pending: the caller may destroy that stream, the next encode waits for nothing
    return FIC_OK;
}

int SweepTimer::flush()
{
    for (size_t i = 0; i + 1 < ev.size(); i += 2) {
        HIP_TRY(hipEventSynchronize(ev[i + 1]));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
        acc_ms += ms;
        acc_n += 1;
        (void)hipEventDestroy(ev[i]);
        (void)hipEventDestroy(ev[i + 1]);
    }
    ev.clear();
    return FIC_OK;
}
int SweepTimer::begin(hipStream_t s)
{
    if (!on) return FIC_OK;
    if (ev.size() >= 256) {                            // bound the pending list: fold finished launches into the accumulators
        int rc = flush();
        if (rc) return rc;
    }
    return end(s);
}
int SweepTimer::end(hipStream_t s)
{
    if (!on) return FIC_OK;
    hipEvent_t e = nullptr;
    HIP_TRY(hipEventCreate(&e));
    ev.push_back(e);
    HIP_TRY(hipEventRecord(e, s));
    return FIC_OK;
}
int SweepTimer::read(double* total_ms, int* launches, int reset)
{
    int rc = flush();
    if (rc) return rc;
    if (total_ms) *total_ms = acc_ms;
    if (launches) *launches = acc_n;
    if (reset) { acc_ms = 0.0; acc_n = 0; }
    return FIC_OK;
}

int grow_lsq_slots(CtxCore* c, void*& slotE, uint32_t*& slotC, size_t nslots, size_t sizeE, size_t sizeC)
{
    if (c->lsq_slots >= nslots) return FIC_OK;
    HIP_TRY(hipStreamSynchronize(c->last_stream));
    c->mem.release(slotE);
    c->mem.release(slotC);
    c->lsq_slots = 0;
    int rc = c->mem.ensure(slotE, sizeE);
    if (rc == FIC_OK) rc = c->mem.ensure(slotC, sizeC);
    if (rc) return rc;
    c->lsq_slots = nslots;
    return FIC_OK;
}

int debug_store_host(CtxCore* c, const char* who, const void* const* stores, int nstores, int which, void* out, int64_t capacity, int64_t* size)
{
    if (which < 0 || which >= nstores) return fail(FIC_E_ARGUMENT, "%s: which must be 0..%d", who, nstores - 1);
    const void* src = stores[which];
    const size_t bytes = c->mem.bytes_of(src);          // the stores exactly as the owner holds them
    *size = (int64_t)bytes;
    if (!out) return FIC_OK;
    if (capacity < (int64_t)bytes) return fail(FIC_E_CAPACITY, "%s: %zu bytes needed", who, bytes);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->last_stream));
    HIP_TRY(hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost));
    return FIC_OK;
}

// "sweep_stats": the counter block is switched on (zeroed) or off
static int sweep_stats_option(CtxCore* c, int on)
{
    HIP_TRY(hipSetDevice(c->device));
    if (on && !c->sweep_stats) {
        int rc = c->mem.ensure_zeroed(c->sweep_stats, 8, nullptr);
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(nullptr));            // the fill is only enqueued (null stream); sweeps run on other streams
    } else if (!on && c->sweep_stats) {
        HIP_TRY(hipStreamSynchronize(c->last_stream));
        c->mem.release(c->sweep_stats);
    }
    return FIC_OK;
}

int set_core_option(CtxCore* c, int handle, const char* prefix, const char* name, int value)
{
    const OptionRule* r = find_option(name, handle);
    if (!r) return fail(FIC_E_ARGUMENT, "%sunknown option '%s'", prefix, name);
    if (!option_value_ok(*r, value)) return fail(FIC_E_ARGUMENT, "%s%s %s", prefix, r->name, r->must);
    switch (r->id) {
    case kOptSearch: c->opt_search = value; break;
    case kOptChunks: c->opt_chunks = value; break;
    case kOptQEshift: c->g.q_eshift = value; break;
    case kOptLsqTauWiden: c->opt_lsq_widen = value; break;
    case kOptLsqEngine: c->opt_lsq_engine = value; break;
    case kOptLsqQEshift: c->opt_lsq_q_eshift = value; break;
    case kOptTimeSweep: c->timer.on = value ? 1 : 0; break;
    case kOptSweepStats: return sweep_stats_option(c, value);
    }
    return FIC_OK;
}

int ctx_get_lsq_error(CtxCore* c, const char* who, int64_t* E)
{
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->encoded_any || c->last_search != 1 || !c->lsq_E)
        return fail(FIC_E_STATE, "%s: the last encode was not a least-squares search (\"search\" = 1)", who);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->last_stream));
    static_assert(sizeof(long long) == sizeof(int64_t), "E");
    HIP_TRY(hipMemcpy(E, c->lsq_E, (size_t)c->g.planes * c->g.Nr * sizeof(int64_t), hipMemcpyDeviceToHost));
    return FIC_OK;
}

int ctx_sweep_time(CtxCore* c, double* total_ms, int* launches, int reset)
{
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    return c->timer.read(total_ms, launches, reset);
}

int ctx_sweep_stats(CtxCore* c, const char* who, uint64_t* out8, int reset)
{
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->sweep_stats) return fail(FIC_E_STATE, "%s: set the option \"sweep_stats\" first", who);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->last_stream));
    HIP_TRY(hipMemcpy(out8, c->sweep_stats, 8 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (reset) {
        HIP_TRY(hipMemset(c->sweep_stats, 0, 8 * sizeof(uint64_t)));
        HIP_TRY(hipStreamSynchronize(nullptr));
    }
    return FIC_OK;
}

int ctx_debug_lsq_q(CtxCore* c, const char* who, int which, void* out, int64_t capacity, int64_t* size)
{
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->encoded_any || !c->lsq_q[0])
        return fail(FIC_E_STATE, "%s: no encode through the matrix-core least-squares sweep (\"lsq_engine\" = 1) yet", who);
    return debug_store_host(c, who, c->lsq_q, 4, which, out, capacity, size);
}

int upload_bytes(CtxCore* c, void* own, const void* host, size_t bytes)
{
    HIP_TRY(hipStreamSynchronize(c->last_stream));     // an earlier encode on a non-blocking stream may still read the copy
    HIP_TRY(hipMemcpy(own, host, bytes, hipMemcpyHostToDevice));
    return FIC_OK;
}

int upload_argb_as_gray(CtxCore* c, int32_t*& stage, uint8_t*& gray_own, const int32_t* argb, size_t npix)
{
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = c->mem.ensure(gray_own, npix)) return rc;
    if (int rc = c->mem.ensure(stage, npix)) return rc;
    if (int rc = upload_bytes(c, stage, argb, npix * sizeof(int32_t))) return rc;
    if (fic_launch_argb_to_gray(stage, gray_own, npix, nullptr)) return fail(FIC_E_HIP, "k_argb_to_gray launch failed");
    HIP_TRY(hipStreamSynchronize(nullptr));
    c->have_input = true;
    return FIC_OK;
}

int check_input_alignment(const char* entry, const void* dev, int align)
{
    if ((uintptr_t)dev % (uintptr_t)align == 0) return FIC_OK;
    return fail(FIC_E_ARGUMENT, "%s: alignment: address %p is not a multiple of %d bytes (the input in force stays)", entry, dev, align);
}

}  // namespace ficd
