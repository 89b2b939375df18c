// fic_ctx_core.cpp -- what fic_ctx and fic_rgb_ctx do alike, over the core they share (ficd::CtxCore, fic_internal.h): the
// stream rule, the sweep timer, the growth of the least-squares slot stores, the read-out of a debug store, the sync entry and
// the "sweep_stats" counter block.  Host-side orchestration only.
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

int sweep_stats_option(CtxCore* c, unsigned long long*& stats, int on)
{
    HIP_TRY(hipSetDevice(c->device));
    if (on && !stats) {
        int rc = c->mem.ensure_zeroed(stats, 8, nullptr);
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(nullptr));            // the fill is only enqueued (null stream); sweeps run on other streams
    } else if (!on && stats) {
        HIP_TRY(hipStreamSynchronize(c->last_stream));
        c->mem.release(stats);
    }
    return FIC_OK;
}

int sweep_stats_read(CtxCore* c, const char* who, unsigned long long* stats, uint64_t* out8, int reset)
{
    if (!stats) return fail(FIC_E_STATE, "%s: set the option \"sweep_stats\" first", who);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->last_stream));
    HIP_TRY(hipMemcpy(out8, stats, 8 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (reset) {
        HIP_TRY(hipMemset(stats, 0, 8 * sizeof(uint64_t)));
        HIP_TRY(hipStreamSynchronize(nullptr));
    }
    return FIC_OK;
}

}  // namespace ficd
