// fic_internal.h -- shared by the translation units of the C ABI that call HIP (fic_capi*.cpp): the context types and the core
// they share (fic_ctx_core.cpp: stream rule, options, host input, the getters that differ only in the handle type), the
// idle-context caches of the one-shot entries and the lease on them, the decode job and the release hooks; error
// reporting, geometry validation and the stream formats come with fic_stream.h, the ownership of device memory with
// fic_devmem.h (the HIP runtime's allocation calls are made in fic_devmem.cpp and nowhere else).  Not part of the public
// interface.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <functional>
#include <initializer_list>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/fic.h"
#include "fic_device.h"
#include "fic_launch.h"
#include "fic_stream.h"
#include "fic_devmem.h"
#include "fic_qt_batch_plan.h"
#include "fic_ctx_options.h"

struct fic_rgb_ctx;

namespace ficd {

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return ficd::fail(FIC_E_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// keeps the calling thread's error across clean-up calls that may overwrite it
struct ErrKeep {
    std::string msg = g_err;
    int code = g_err_code;
    ~ErrKeep() { g_err = msg; g_err_code = code; }
};

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// Makes `device` current, or refuses it with FIC_E_NO_DEVICE (fic_capi.cpp)
int check_device(int device);
// The device check of the two *_create entries: records why and returns false, or makes `device` current (fic_capi.cpp)
bool create_device_ok(int device);

int encode_oneshot(const uint8_t* gray, const int32_t* argb, int w, int h, int B, int wK, int n_iso, int device,
                   int32_t* idx_local, float* a, float* b, int32_t* iso, int32_t* qrows, int64_t* E = nullptr, int search = 0);

// "time_sweep": event pairs bracket the sweep launch on its stream and are read later (fic_*_ctx_sweep_time).
struct SweepTimer {
    int on = 0;                      // the option; while it is off no event is created
    std::vector<hipEvent_t> ev;      // pending pairs start/stop
    double acc_ms = 0.0;
    int acc_n = 0;
    int begin(hipStream_t s);        // folds the pending list into the accumulators first once it holds 256 events
    int end(hipStream_t s);
    int flush();                     // waits for the pending pairs and adds them up
    int read(double* total_ms, int* launches, int reset);
};

// What a context is apart from its pixels: fic_ctx, fic_rgb_ctx and fic_qt_ctx derive from it, the helpers below
// (fic_ctx_core.cpp) are written once for all of them.
struct CtxCore {
    int device = 0;
    FicGeom g;
    DevMem mem;                      // owns every device and pinned pointer of the context
    std::mutex mu;
    bool have_input = false, encoded_any = false;
    hipStream_t last_stream = nullptr;
    bool stream_used = false;        // an encode was issued on last_stream (take_stream orders a stream switch after it)
    SweepTimer timer;
    size_t lsq_slots = 0;            // slots per plane the least-squares slot stores have room for
    // the shared options (fic_ctx_options.h; "q_eshift" is g.q_eshift, "time_sweep" timer.on) and what the last encode ran
    int opt_search = 0, last_search = 0;
    int opt_chunks = 0;              // pool chunks of the sweep (0 = automatic)
    int opt_lsq_widen = 0;           // "lsq_tau_widen" (0 or 8..24): diagnostic, > 0 gives WRONG codebooks
    int opt_lsq_engine = 0;          // "lsq_engine": 1 the matrix-core least-squares sweep wherever the fast VALU one would run
    int opt_lsq_q_eshift = 0;        // "lsq_q_eshift" (-12..4): diagnostic, that sweep's Er times 2^-value; > 0 gives WRONG codebooks
    unsigned long long* sweep_stats = nullptr;   // "sweep_stats" = 1: 8 u64 device counters of the matrix-core sweeps
    // stores of a least-squares search the shared getters read; a context's FicLsq* / FicLsq*Q structs view them for the launchers
    void* lsq_E = nullptr;           // the winners' E, i64 [planes][Nr]
    void* lsq_q[4] = {};             // "lsq_engine" = 1: poolQ, rngQ, rngE, rngR
    ~CtxCore();                      // the pending events; the memory goes with `mem`
};

// Stream rule of the handle API (include/fic.h), in this one place: an encode on stream `s` takes over the
// context.  On the stream of the encode before it this is one pointer comparison; on another one the host waits for the earlier
// encode first, since stream order no longer keeps the two apart.  Afterwards last_stream is `s` and nothing reads any other
// stream.  (The multi-device entry sets last_stream itself, after its own wait: fic_capi_multi.cpp.)
int take_stream(CtxCore* c, hipStream_t s);
// fic_*_ctx_sync: waits for last_stream; nothing is pending then, the caller may destroy that stream
int ctx_sync(CtxCore* c);
// Room for `nslots` slots per plane in the two slot stores of a least-squares search (sizeE, sizeC as DevMem::ensure counts
// them); growing waits for last_stream, whose sweep may still use the old stores
int grow_lsq_slots(CtxCore* c, void*& slotE, uint32_t*& slotC, size_t nslots, size_t sizeE, size_t sizeC);
// The fic_*_debug_*_host entries behind their own preconditions: store `which` of `stores` exactly as the owner holds it
int debug_store_host(CtxCore* c, const char* who, const void* const* stores, int nstores, int which, void* out, int64_t capacity, int64_t* size);
// One of the shared options (fic_ctx_options.h) of handle kind `handle` (OptHandle): range check and effect; a name the table
// does not list for that handle is the unknown option.  `prefix` opens every message ("" for the grey entry).  The caller
// holds c->mu.
int set_core_option(CtxCore* c, int handle, const char* prefix, const char* name, int value);
// The getters that differ only in the handle type, behind the entry's null check (`who`: the entry's name); they take c->mu.
int ctx_get_lsq_error(CtxCore* c, const char* who, int64_t* E);
int ctx_sweep_time(CtxCore* c, double* total_ms, int* launches, int reset);
int ctx_sweep_stats(CtxCore* c, const char* who, uint64_t* out8, int reset);
int ctx_debug_lsq_q(CtxCore* c, const char* who, int which, void* out, int64_t capacity, int64_t* size);
// Host input: upload_input ensures the context's copy `own`, waits until last_stream no longer reads it, copies `count`
// elements from `host` (upload_bytes) and sets have_input; upload_argb_as_gray does the same for an ARGB image's red channel,
// through the staging copy `stage` and k_argb_to_gray on the null stream.  The caller holds c->mu.
int upload_bytes(CtxCore* c, void* own, const void* host, size_t bytes);
int upload_argb_as_gray(CtxCore* c, int32_t*& stage, uint8_t*& gray_own, const int32_t* argb, size_t npix);
template <typename T>
int upload_input(CtxCore* c, T*& own, const T* host, size_t count)
{
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = c->mem.ensure(own, count)) return rc;
    if (int rc = upload_bytes(c, own, host, count * sizeof(T))) return rc;
    c->have_input = true;
    return FIC_OK;
}
// Device input: FIC_OK, or the refusal of an address that is no multiple of `align` bytes (nothing of the context has changed)
int check_input_alignment(const char* entry, const void* dev, int align);


// device arena of a decode (fic_capi_decode.cpp): one allocation kept between calls, taken and given back by a DecodeJob
struct Arena {
    int device = -1;
    size_t bytes = 0;
    char* base = nullptr;
};
// What the two decoders of the reference differ in around their loop: the pixel of generateGrayImage (FC:1142-1148) the image
// starts from, and the names a row outside the pool is reported with.
struct DecodeKind {
    size_t px_bytes;         // 1: grey bytes, 4: packed ARGB
    uint32_t px_start;
    const char* name;
    const char* paint_line;  // where the reference throws ArrayIndexOutOfBounds
};
constexpr DecodeKind kDecodeGrey{1, 128u, "decode", "FC:394"}, kDecodeRgb{4, 0xff808080u, "decodeRGB", "FC:477"};

// The device side of one decode of g.planes images on the geometry g (fic_capi_decode.cpp): the workspace of the loop --
// the scaled copy [planes][Hs][Ws] and the image [planes][H][W] in pixels of kind.px_bytes, the loop state [planes], sqbuf --
// and the int32 spans uploaded for it (rows, isometries, per-level leaf lists).  The workspace is carved from an arena
// (open) or is the caller's (borrow: the contexts' zoom-1 decodes); an arena goes back when the job goes out of scope.
struct DecodeJob {
    const DecodeKind* kind = nullptr;
    FicGeom g{};
    hipStream_t stream = nullptr;        // the null stream for the stream decoders, a context's last_stream
    void *scaled = nullptr, *image = nullptr;
    FicDecodeState* state = nullptr;
    uint32_t* sq = nullptr;
    std::vector<const int32_t*> spans;   // the device copies of open()'s `upload`, in its order
    Arena arena;
    DecodeJob() = default;
    DecodeJob(const DecodeJob&) = delete;
    DecodeJob& operator=(const DecodeJob&) = delete;
    ~DecodeJob();
    // the caller has made `device` current
    int open(const char* who, int device, const DecodeKind& kind, const FicGeom& g, hipStream_t s,
             std::initializer_list<const std::vector<int32_t>*> upload = {});
    void borrow(const DecodeKind& kind, const FicGeom& g, hipStream_t s, void* scaled, void* image, FicDecodeState* state, uint32_t* sq);
    // The decoder's loop (decodeGreyScale FC:381-418, decodeRGB FC:458-505) around `iteration(counter)`, which enqueues one
    // iteration -- scale, paint, fic_launch_decode_step -- on `stream`; then the image [planes][H][W] to host_out.  avg_in
    // [planes]: avgError carried in (NULL: 0); avg_out / iters_out / seq_out [planes] may be NULL and may alias avg_in.  On
    // failure nothing of the caller's is written.
    int run(const char* who, const float* avg_in, float* avg_out, int* iters_out, int* seq_out, void* host_out,
            const std::function<int(int)>& iteration);
};

// The encode of a colour context under "search" = 1 (fic_capi_rgb_lsq.cpp); the caller holds the context's lock, has made its
// device current and taken the stream (take_stream)
int rgb_lsq_encode(fic_rgb_ctx* c, int with_collage, hipStream_t s);

// The quadtree encode behind the level encodes (fic_capi_quadtree.cpp), one pipeline for the one-shot entries
// (a plan of one plane) and the batched handle: the per-level SSE, the rule's keys and select, the compaction and, if asked
// for, the tree statistics, all enqueued on s.  Every area lies in `store` where the plan Q says, and every parameter of the
// rule is read there by the kernels: the threshold's bits or a given lambda in kQtParam, the rank of a leaf budget (qt_rank) in
// kQtRanks, an SSE target in kQtValues; the caller has put it there on s.  Results: kQtLeaves, kQtNLeaves, kQtParam, kQtStats.
// views [L.nl]: the device arrays of every level's encode, whoever made them.  goal: FIC_QT_RD_* under kRuleRd.
enum QtRule { kRuleThreshold, kRuleBudget, kRuleRd };
template <typename Px>
struct QtViews {
    const Px *image, *scaled;         // the input [planes][H][W] and the 2:1 copy [planes][Hs][Ws] the rows refer to
    const int32_t *qrows, *iso;
};
template <typename Dev>
int qt_tree_run(const char* kind, const QtBatchPlan& Q, char* store, const QtLevels& L, const QtViews<typename Dev::Px>* views, QtRule rule,
                int goal, bool stats, hipStream_t s);
// the rank of the select for a budget of M >= Ntop leaves: S = (M - Ntop) / 3 blocks may split, the block of rank S must not
inline uint32_t qt_rank(uint64_t M, const QtBatchPlan& Q)
{
    const uint64_t S = (M - (uint64_t)Q.Ntop) / 3;
    return (uint32_t)(S < (uint64_t)Q.nkeys ? S : (uint64_t)Q.nkeys);
}

// what fic_release_cache() frees besides the idle contexts
void release_decoder_arenas();     // fic_capi_decode.cpp
void release_comms();              // fic_capi_multi.cpp

}  // namespace ficd

// Device-resident working set of `planes` grey images of one geometry on one device (fic_ctx_* of include/fic.h).
struct fic_ctx : ficd::CtxCore {
    FicBuffers b;                    // b, o and lsq view what `mem` holds
    FicOutputs o;
    uint8_t* gray_own = nullptr;     // context-owned input copy
    int32_t* argb_stage = nullptr;   // staging for ARGB uploads
    int32_t* collage = nullptr;
    int32_t* host_rec = nullptr;     // pinned host copy of the packed records (fic_ctx_get_results_host)
    uint8_t* decoded = nullptr;      // decoder output image(s)
    FicDecodeState* dec_state = nullptr;   // decoder loop state [planes] and per-pixel squared changes [planes][W*H]
    uint32_t* dec_sq = nullptr;
    void* mfma_poolB = nullptr;      // opt-in matrix-core sweep: B fragments, A fragments, range constants
    void* mfma_rngA = nullptr;
    void* mfma_sw = nullptr;
    int* mfma_rconst = nullptr;
    int mfma_bf16 = 0;               // operand type the fragment stores were built for
    void* q_pool = nullptr;          // k_sweep_q ("sweep" = 6): A fragments, flat-tile flags, B fragments, error bounds, published theta
    void* q_flat = nullptr;
    void* q_rng = nullptr;
    void* q_rngC = nullptr;                  // the sweep columns' isometry copies as bytes (exact evaluation of flagged pairs)
    void* q_E = nullptr;
    void* q_thg = nullptr;
    unsigned int* q_fin = nullptr;           // fused finalise of small launches: finished workgroups per (plane, column group)
    uint32_t* d4_rng = nullptr;      // k_sweep_d4: range / domain slots of the group-Fourier form (n_iso = 8, B = 8 / 16)
    uint32_t* d4_pool = nullptr;
    FicLsq lsq{};                    // least-squares search ("search" = 1): statistics, per-chunk slots, the winners' E (on first use)
    FicLsqQ lsqq{};                  // the matrix-core least-squares sweep k_sweep_lsq_q ("lsq_engine" = 1): fragments, Er, R (on first use)
    hipStream_t own_stream = nullptr; // non-blocking stream of the multi-device entry (created on demand)
    int opt_sweep = 0, opt_noflag = 0;
    int last_chunks = 0, last_kind = 0, last_fused = 0, last_tiles_per_chunk = 0;
    ~fic_ctx();                      // the own stream (fic_capi.cpp)
};

// Device-resident working set of `planes` colour images of one geometry (fic_rgb_ctx_* of include/fic.h, fic_capi_rgb.cpp).
// The kernels take the image from their grid: a batch is one launch per stage on the caller's stream (only the matrix-core
// full search runs image by image).
struct fic_rgb_ctx : ficd::CtxCore {
    int32_t* argb_own = nullptr;     // context-owned input copy
    const int32_t* argb = nullptr;   // input in use (own copy or the caller's device pointer)
    int32_t* scaled = nullptr;       // per plane: [H/2][W/2]
    uint16_t* pool_sum = nullptr;    // [N_d][n]
    float* pool_cf = nullptr;        // [N_d][n] (full search at B = 4 / 8)
    FicRgbDomStat* pool_st = nullptr;
    int16_t* rng_t = nullptr;
    FicRgbRngStat* rng_st = nullptr;
    unsigned long long* key = nullptr;
    int32_t *idx_local = nullptr, *idx_global = nullptr, *qrows = nullptr, *collage = nullptr;
    float *a = nullptr, *bR = nullptr, *bG = nullptr, *bB = nullptr;
    int32_t* iso = nullptr;          // winning isometries [planes][N_r] (n_iso = 8 contexts only; g.n_iso says which)
    int32_t* dec_image = nullptr;    // decoder: image, scaled image, state, per-pixel squared changes (one plane at a time)
    int32_t* dec_scaled = nullptr;
    FicDecodeState* dec_state = nullptr;
    uint32_t* dec_sq = nullptr;
    FicRgbQ q;                       // matrix-core full search (allocated on first use; one image at a time, stream-ordered)
    int opt_sweep = 0;               // 0 auto, 1 VALU sweeps, 2 matrix-core full search
    int last_sweep = 0;              // what the last encode ran: 1 / 2
    FicLsqRgb lsq;                   // least-squares search ("search" = 1): byte stores, sums, per-chunk slots, the winners' E (on first use)
    int last_lsq_kind = 0;           // the least-squares sweep the last encode ran: 1 generic, 2 fast, 7 matrix cores (k_sweep_lsq_rgb_q)
    FicLsqRgbQ lsqq{};               // the matrix-core least-squares sweep k_sweep_lsq_rgb_q ("lsq_engine" = 1): fragments, Er, R (on first use)
    int last_lsq_chunks = 0;         // pool chunks of the last least-squares sweep
    bool have_collage = false;
};

namespace ficd {

// Idle single-image contexts of the one-shot entries, most recently used last; the oldest is destroyed when a give() finds
// every slot taken.  The grey cache has 16 slots (the multi-device entry parks one context per device), the joint-RGB one 4.
inline void destroy_ctx(fic_ctx* c) { fic_ctx_destroy(c); }
inline void destroy_ctx(fic_rgb_ctx* c) { fic_rgb_ctx_destroy(c); }
template <typename Ctx, size_t kSlots>
class IdleCache {
public:
    Ctx* take(int device, int w, int h, int B, int wK, int n_iso)
    {
        std::lock_guard<std::mutex> lk(mu_);
        for (size_t i = idle_.size(); i-- > 0;) {
            Ctx* c = idle_[i];
            const FicGeom& g = c->g;
            if (c->device == device && g.W == w && g.H == h && g.B == B && g.wK == wK && g.n_iso == n_iso && g.planes == 1) {
                idle_.erase(idle_.begin() + (long)i);
                return c;
            }
        }
        return nullptr;
    }
    void give(Ctx* c)
    {
        Ctx* evict = nullptr;
        {
            std::lock_guard<std::mutex> lk(mu_);
            idle_.push_back(c);
            if (idle_.size() > kSlots) {
                evict = idle_.front();
                idle_.erase(idle_.begin());
            }
        }
        if (evict) destroy_ctx(evict);
    }
    void drain()
    {
        std::vector<Ctx*> drop;
        {
            std::lock_guard<std::mutex> lk(mu_);
            drop.swap(idle_);
        }
        for (Ctx* c : drop) destroy_ctx(c);
    }

private:
    std::mutex mu_;
    std::vector<Ctx*> idle_;
};
extern IdleCache<fic_ctx, 16> g_idle_grey;       // fic_capi.cpp
extern IdleCache<fic_rgb_ctx, 4> g_idle_rgb;     // fic_capi_rgb.cpp
inline IdleCache<fic_ctx, 16>& idle_cache(fic_ctx*) { return g_idle_grey; }
inline IdleCache<fic_rgb_ctx, 4>& idle_cache(fic_rgb_ctx*) { return g_idle_rgb; }
inline fic_ctx* create_ctx(fic_ctx*, int device, int w, int h, int B, int wK, int n_iso) { return fic_ctx_create(device, w, h, B, wK, n_iso, 1); }
inline fic_rgb_ctx* create_ctx(fic_rgb_ctx*, int device, int w, int h, int B, int wK, int n_iso) { return fic_rgb_ctx_create_iso(device, w, h, B, wK, n_iso, 1); }

// The lease of a one-shot entry on a single-image context: open() takes an idle one of the geometry or creates it, and may put
// it under "search" = 1 for the call.  close(rc) ends it: the context is back in the reference's mode -- the cached contexts
// serve the reference entries too -- and goes to the cache if rc is FIC_OK, else it is destroyed, as is one whose lease goes out
// of scope open.  The calling thread's error stays what it was across that clean-up.
template <typename Ctx>
class Lease {
public:
    Ctx* c = nullptr;
    Lease() = default;
    Lease(const Lease&) = delete;
    Lease& operator=(const Lease&) = delete;
    int open(int device, int w, int h, int B, int wK, int n_iso, int search = 0)
    {
        c = idle_cache(c).take(device, w, h, B, wK, n_iso);
        if (!c) c = create_ctx(c, device, w, h, B, wK, n_iso);
        if (!c) return g_err_code ? g_err_code : FIC_E_HIP;   // the creator recorded why
        c->opt_search = search;
        return FIC_OK;
    }
    int close(int rc)                // ends the lease with what the entry returns: the context is kept after success only
    {
        finish(rc == FIC_OK);
        return rc;
    }
    ~Lease() { finish(false); }

private:
    void finish(bool ok)
    {
        if (!c) return;
        ErrKeep keep;
        c->opt_search = 0;
        if (ok) idle_cache(c).give(c);
        else destroy_ctx(c);
        c = nullptr;
    }
};

}  // namespace ficd
