// devmem_test.cpp -- the owner of device memory (csrc/fic_devmem.h) under the host compiler's sanitizers.  Stand-alone: the
// header's binding is defined here on malloc / free, with a switch that makes the k-th allocation fail, so the bookkeeping the
// contexts of the C ABI rely on runs with no HIP and no GPU (tests/test_devmem.py builds this file and fic_stream.cpp with
// -fsanitize=address,undefined and runs it).  A block the owner forgets is the leak checker's to report: the program frees
// nothing behind the owner's back.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../fractal-image-compression_amd/csrc/fic_devmem.h"

using namespace ficd;

namespace {

int g_failures = 0, g_checks = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        g_checks++;                                        \
        if (!(cond)) {                                     \
            g_failures++;                                  \
            fprintf(stderr, "%s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);                  \
            fprintf(stderr, "\n");                         \
        }                                                  \
    } while (0)

// the malloc-backed binding
int g_alloc_calls = 0;       // raw_alloc calls so far
int g_fail_at = 0;           // the call (1-based) that fails; 0: none
int g_raw_live = 0;          // blocks handed out and not yet freed
int g_last_device = -1;      // what raw_use_device was last told
int g_zero_calls = 0;

int64_t live(int i) { return g_mem_live[i].load(); }
bool all_zero() { return !live(0) && !live(1) && !live(2) && !live(3); }

struct Stat { int a, b; };   // an element type of 8 bytes

}  // namespace

int ficd::raw_alloc(MemKind, void** p, size_t bytes, const char** why)
{
    if (++g_alloc_calls == g_fail_at) {
        *why = "out of memory (injected)";
        return 1;
    }
    *p = malloc(bytes ? bytes : 1);
    if (!*p) { *why = "malloc failed"; return 1; }
    memset(*p, 0xA5, bytes);                     // an overrun of `bytes` is the sanitizer's to report
    g_raw_live++;
    return 0;
}
void ficd::raw_free(MemKind, void* p) { free(p); g_raw_live--; }
void ficd::raw_use_device(int device) { g_last_device = device; }
int ficd::raw_zero_async(void* p, size_t bytes, void*) { memset(p, 0, bytes); g_zero_calls++; return 0; }

namespace {

void test_ensure_release_bytes_of()
{
    DevMem m(3);
    uint8_t* a = nullptr;
    Stat* s = nullptr;
    void* v = nullptr;
    CHECK(m.ensure(a, 100) == FIC_OK && a, "ensure");
    CHECK(m.ensure(s, 10) == FIC_OK && s, "ensure typed");
    CHECK(m.ensure(v, 77) == FIC_OK && v, "ensure untyped");
    CHECK(m.bytes_of(a) == 100 && m.bytes_of(s) == 10 * sizeof(Stat) && m.bytes_of(v) == 77, "bytes_of: %zu %zu %zu", m.bytes_of(a), m.bytes_of(s), m.bytes_of(v));
    CHECK(live(0) == 100 + 80 + 77 && live(1) == 3 && live(2) == 0 && live(3) == 0, "counters %lld %lld", (long long)live(0), (long long)live(1));
    // ensure is idempotent: same pointer, no call of the binding, no new record
    uint8_t* const a0 = a;
    const int calls = g_alloc_calls;
    CHECK(m.ensure(a, 100) == FIC_OK && a == a0 && m.ensure(a, 5000) == FIC_OK && a == a0, "ensure on a set pointer moved it");
    CHECK(g_alloc_calls == calls && (size_t)(live(1) + live(3)) == 3 && live(1) == 3 && m.bytes_of(a) == 100, "ensure on a set pointer allocated");
    a[99] = 1;                                   // usable to its last byte
    s[9].b = 2;
    // bytes_of answers for live allocations only: not for null, an interior pointer, a foreign pointer or a released one
    int on_stack = 0;
    CHECK(m.bytes_of(nullptr) == 0 && m.bytes_of(a + 1) == 0 && m.bytes_of(&on_stack) == 0, "bytes_of of something not held");
    // release nulls the pointer, frees on the owner's device and takes the counters down
    g_last_device = -1;
    m.release(s);
    CHECK(s == nullptr && g_last_device == 3, "release: pointer %p, device %d", (void*)s, g_last_device);
    CHECK(live(0) == 177 && live(1) == 2 && (size_t)(live(1) + live(3)) == 2 && g_raw_live == 2, "release: counters %lld %lld", (long long)live(0), (long long)live(1));
    m.release(s);                                // a null pointer: nothing happens
    Stat* foreign = (Stat*)&on_stack;            // not the owner's: nulled, not freed
    m.release(foreign);
    CHECK(foreign == nullptr && (size_t)(live(1) + live(3)) == 2 && g_raw_live == 2, "release of a pointer the owner does not hold");
    // release then ensure: a new store of the new size (the operand-type switch, the slot growth)
    m.release(a);
    CHECK(m.bytes_of(a0) == 0, "bytes_of of a released pointer");
    CHECK(m.ensure(a, 300) == FIC_OK && a && m.bytes_of(a) == 300 && live(0) == 377, "release + ensure");
    // pinned memory is counted on its own
    int32_t* h = nullptr;
    CHECK(m.ensure(h, 6, kMemPinned) == FIC_OK && m.bytes_of(h) == 24 && live(2) == 24 && live(3) == 1 && live(1) == 2, "pinned counters");
    // allocate-and-zero: zeroed once, when allocated
    uint32_t* z = nullptr;
    const int zc = g_zero_calls;
    CHECK(m.ensure_zeroed(z, 16, nullptr) == FIC_OK && z && g_zero_calls == zc + 1, "ensure_zeroed");
    bool zero = true;
    for (int i = 0; i < 16; i++) zero = zero && z[i] == 0;
    z[3] = 7;
    CHECK(zero && m.ensure_zeroed(z, 16, nullptr) == FIC_OK && z[3] == 7 && g_zero_calls == zc + 1, "ensure_zeroed filled again");
    // reset frees everything and the owner can be used again
    m.reset();
    CHECK(all_zero() && g_raw_live == 0 && (size_t)(live(1) + live(3)) == 0, "reset left %d blocks", g_raw_live);
    a = nullptr;
    CHECK(m.ensure(a, 8) == FIC_OK && live(1) == 1, "ensure after reset");
}   // destruction frees the last one

// ten allocations, the k-th fails: the earlier ones stay usable, the failed pointer is null, a retry succeeds
void test_failing_allocation(int k)
{
    const int N = 10;
    g_alloc_calls = 0;
    g_fail_at = k;
    {
        DevMem m(0);
        uint32_t* p[N] = {};
        int first_bad = -1;
        for (int i = 0; i < N; i++) {
            const int rc = m.ensure(p[i], (size_t)(i + 1) * 11);
            if (rc && first_bad < 0) first_bad = i;
            CHECK(rc == (i == k - 1 ? FIC_E_HIP : FIC_OK), "k=%d: allocation %d returned %d", k, i, rc);
        }
        CHECK(first_bad == k - 1 && p[k - 1] == nullptr, "k=%d: failed pointer %p", k, (void*)p[k - 1]);
        CHECK(strstr(g_err.c_str(), "injected") && !strcmp(g_mem_why, "out of memory (injected)") && g_err_code == FIC_E_HIP, "k=%d: error '%s'", k, g_err.c_str());
        CHECK((size_t)(live(1) + live(3)) == (size_t)N - 1 && live(1) == N - 1 && g_raw_live == N - 1, "k=%d: %zu held", k, (size_t)(live(1) + live(3)));
        for (int i = 0; i < N; i++)
            if (i != k - 1) {
                p[i][0] = 1;
                p[i][(i + 1) * 11 - 1] = 2;                                   // every other store is whole
                CHECK(m.bytes_of(p[i]) == (size_t)(i + 1) * 44, "k=%d: bytes_of %d", k, i);
            }
        CHECK(m.ensure(p[k - 1], (size_t)k * 11) == FIC_OK && p[k - 1] && (size_t)(live(1) + live(3)) == (size_t)N, "k=%d: the retry failed", k);
        p[k - 1][k * 11 - 1] = 3;
        int64_t want = 0;
        for (int i = 0; i < N; i++) want += (i + 1) * 44;
        CHECK(live(0) == want && live(1) == N, "k=%d: %lld bytes live, expected %lld", k, (long long)live(0), (long long)want);
    }
    g_fail_at = 0;
    CHECK(all_zero() && g_raw_live == 0, "k=%d: destruction left %d blocks", k, g_raw_live);
}

// one-call scratch: an owner on the stack frees on every way out of the call
int scratch_call(int fail_second)
{
    DevMem scratch(1);
    char* a = nullptr;
    float* b = nullptr;
    int rc = scratch.alloc(a, 64);
    if (rc) return rc;
    g_fail_at = fail_second ? g_alloc_calls + 1 : 0;
    rc = scratch.alloc(b, 8);
    g_fail_at = 0;
    if (rc) return rc;                           // the early return: `a` goes with the owner
    b[7] = 1.0f;
    return FIC_OK;
}

// the pair used without an owner (the decoders' arenas, the multi-device staging buffer)
void test_pair()
{
    void* p = nullptr;
    CHECK(mem_alloc(kMemPinnedPortable, &p, 4096) == FIC_OK && p && live(2) == 4096 && live(3) == 1 && live(0) == 0, "pair: pinned");
    mem_free(kMemPinnedPortable, p, 4096);
    mem_free(kMemDevice, nullptr, 123);          // a null pointer is not counted
    CHECK(all_zero(), "pair: counters after free");
    g_fail_at = g_alloc_calls + 1;
    p = &p;
    CHECK(mem_alloc(kMemDevice, &p, 16) == FIC_E_HIP && p == nullptr && all_zero(), "pair: a failed allocation was counted");
    g_fail_at = 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc > 1 && !strcmp(argv[1], "forget")) {
        // what a free left out looks like: an owner that is never destroyed.  The leak checker must end this run with an error.
        DevMem* lost = new DevMem(0);
        uint8_t* p = nullptr;
        if (lost->alloc(p, 1000)) return 0;
        printf("devmem_test: forgot %zu bytes\n", lost->bytes_of(p));
        fflush(stdout);                          // the leak checker ends the process without flushing
        lost = nullptr;
        p = nullptr;
        return 0;
    }
    CHECK(all_zero(), "counters at start");
    test_ensure_release_bytes_of();
    CHECK(all_zero() && g_raw_live == 0, "destruction left %d blocks", g_raw_live);
    for (int k = 1; k <= 10; k++) test_failing_allocation(k);
    CHECK(scratch_call(0) == FIC_OK && all_zero() && g_raw_live == 0, "scratch, success");
    CHECK(scratch_call(1) == FIC_E_HIP && all_zero() && g_raw_live == 0, "scratch, early return");
    test_pair();
    CHECK(all_zero() && g_raw_live == 0, "counters at the end");
    printf("devmem_test: %d checks, %d failures\n", g_checks, g_failures);
    return g_failures ? 1 : 0;
}
