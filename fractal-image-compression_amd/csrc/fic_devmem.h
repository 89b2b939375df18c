// fic_devmem.h -- who owns device (and pinned host) memory under the C ABI.  Every allocation of the library goes
// through the counted pair mem_alloc / mem_free; a DevMem records what it handed out and frees what it still holds when it is
// reset or destroyed.  No HIP: the four raw_* functions are the binding -- fic_devmem.cpp binds them to the HIP runtime's device
// and pinned-host allocation calls, tests/cpp/devmem_test.cpp to malloc.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <atomic>
#include <vector>

#include "fic_stream.h"

namespace ficd {

enum MemKind { kMemDevice = 0, kMemPinned = 1, kMemPinnedPortable = 2 };   // portable: pinned for every device

// ---- the binding: defined once per program -----------------------------------------------------------------------------------
int raw_alloc(MemKind kind, void** p, size_t bytes, const char** why);   // 0, or non-zero with *why = the runtime's words
void raw_free(MemKind kind, void* p);
void raw_use_device(int device);                                         // makes `device` current
int raw_zero_async(void* p, size_t bytes, void* stream);                 // enqueues the fill on `stream` (a hipStream_t)

// ---- the counted pair --------------------------------------------------------------------------------------------------------
inline std::atomic<int64_t> g_mem_live[4];        // live {bytes, allocations} of the process: device, pinned host (fic_debug_live_memory)
inline thread_local const char* g_mem_why = "";   // the runtime's words for the calling thread's last failed mem_alloc

inline int mem_alloc(MemKind kind, void** p, size_t bytes)
{
    *p = nullptr;
    if (raw_alloc(kind, p, bytes, &g_mem_why)) {
        *p = nullptr;
        return fail(FIC_E_HIP, "allocating %zu bytes of %s memory: %s", bytes, kind == kMemDevice ? "device" : "pinned host", g_mem_why);
    }
    g_mem_live[kind == kMemDevice ? 0 : 2] += (int64_t)bytes;
    g_mem_live[kind == kMemDevice ? 1 : 3] += 1;
    return FIC_OK;
}
inline void mem_free(MemKind kind, void* p, size_t bytes)
{
    if (!p) return;
    raw_free(kind, p);
    g_mem_live[kind == kMemDevice ? 0 : 2] -= (int64_t)bytes;
    g_mem_live[kind == kMemDevice ? 1 : 3] -= 1;
}

template <typename T> constexpr size_t mem_elem_bytes() { return sizeof(T); }
template <> constexpr size_t mem_elem_bytes<void>() { return 1; }        // untyped stores are sized in bytes

// ---- the owner ---------------------------------------------------------------------------------------------------------------
// Its records are touched only when something is allocated or released: ensure() on a pointer that is set is one null check.
class DevMem {
public:
    explicit DevMem(int device = -1) : device_(device) {}   // -1: the caller keeps the right device current
    DevMem(const DevMem&) = delete;
    DevMem& operator=(const DevMem&) = delete;
    ~DevMem() { reset(); }
    void set_device(int device) { device_ = device; }

    // `count` elements of T (bytes for T = void) into p, which must not point at memory this owner holds: FIC_OK, or
    // FIC_E_HIP with p == nullptr and everything handed out before still good
    template <typename T>
    int alloc(T*& p, size_t count, MemKind kind = kMemDevice)
    {
        void* v = nullptr;
        recs_.reserve(recs_.size() + 1);                     // nothing can fail between the allocation and its record
        const int rc = mem_alloc(kind, &v, count * mem_elem_bytes<T>());
        if (rc == FIC_OK) recs_.push_back({v, count * mem_elem_bytes<T>(), kind});
        p = (T*)v;
        return rc;
    }
    // no-op when p is set: what `if (!p) allocate` used to spell
    template <typename T>
    int ensure(T*& p, size_t count, MemKind kind = kMemDevice) { return p ? FIC_OK : alloc(p, count, kind); }
    // ensure + on a fresh allocation a zero fill enqueued on `stream` (stores whose padding must stay zero, counters)
    template <typename T>
    int ensure_zeroed(T*& p, size_t count, void* stream)
    {
        if (p) return FIC_OK;
        if (const int rc = alloc(p, count)) return rc;
        return raw_zero_async(p, count * mem_elem_bytes<T>(), stream) ? fail(FIC_E_HIP, "hipMemsetAsync(p, 0, bytes, s) failed") : FIC_OK;
    }
    // frees p if this owner holds it, and nulls it either way
    template <typename T>
    void release(T*& p)
    {
        for (size_t i = recs_.size(); p && i-- > 0;)
            if (recs_[i].p == (const void*)p) {
                free_rec(recs_[i]);
                recs_.erase(recs_.begin() + (long)i);
                break;
            }
        p = nullptr;
    }
    // bytes of the live allocation that starts at p; 0 for anything else
    size_t bytes_of(const void* p) const
    {
        for (const Rec& r : recs_)
            if (p && r.p == p) return r.bytes;
        return 0;
    }
    // frees everything still held (the pointers that viewed it dangle: the caller is done with them)
    void reset()
    {
        for (size_t i = recs_.size(); i-- > 0;) free_rec(recs_[i]);
        recs_.clear();
    }

private:
    struct Rec { void* p; size_t bytes; MemKind kind; };
    void free_rec(const Rec& r) const
    {
        if (device_ >= 0) raw_use_device(device_);
        mem_free(r.kind, r.p, r.bytes);
    }
    std::vector<Rec> recs_;
    int device_;
};

}  // namespace ficd
