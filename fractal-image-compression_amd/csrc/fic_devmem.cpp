// fic_devmem.cpp -- the library's binding of fic_devmem.h: the only translation unit that calls hipMalloc / hipFree /
// hipHostMalloc / hipHostFree, and the debug entry that reports the counters of the pair built on them.
#include <hip/hip_runtime.h>

#include "fic_devmem.h"

namespace ficd {

int raw_alloc(MemKind kind, void** p, size_t bytes, const char** why)
{
    const hipError_t e = kind == kMemDevice ? hipMalloc(p, bytes)
                                            : hipHostMalloc(p, bytes, kind == kMemPinnedPortable ? hipHostMallocPortable : hipHostMallocDefault);
    if (e != hipSuccess) *why = hipGetErrorString(e);
    return e != hipSuccess;
}
void raw_free(MemKind kind, void* p) { (void)(kind == kMemDevice ? hipFree(p) : hipHostFree(p)); }
void raw_use_device(int device) { (void)hipSetDevice(device); }
int raw_zero_async(void* p, size_t bytes, void* stream) { return hipMemsetAsync(p, 0, bytes, (hipStream_t)stream) != hipSuccess; }

}  // namespace ficd

extern "C" int fic_debug_live_memory(int64_t out4[4])
{
    if (!out4) return ficd::fail(FIC_E_ARGUMENT, "fic_debug_live_memory: null argument");
    for (int i = 0; i < 4; i++) out4[i] = ficd::g_mem_live[i].load();
    return FIC_OK;
}
