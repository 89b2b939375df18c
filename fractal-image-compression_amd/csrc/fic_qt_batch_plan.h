// fic_qt_batch_plan.h -- where everything of a batched quadtree context (fic_qt_ctx, fic_capi_qt_ctx.cpp) lies
// in its one device store: the per-plane strides of the batched kernels (fic_quadtree.hip) and the byte offsets of the areas.
// Plain C++ without HIP, integers in and out; tests/cpp/qt_batch_plan_test.cpp runs it under the address and undefined-behaviour
// sanitizers.  Every area starts at a multiple of 256 bytes, no two overlap, `total` is the end of the last one, and every
// element index of the context -- an area's element count, planes included -- stays below 2^31: qt_batch_plan refuses the rest.
#pragma once
#include <stddef.h>
#include <stdint.h>

constexpr int kQtPlanSelectWords = 4 * 256 + 4;     // FIC_QT_SELECT_WORDS = FIC_QT_SELECT_W_WORDS (fic_launch.h)
constexpr int kQtPlanMaxPlanes = 65535;             // the plane is the y dimension of a grid
constexpr int kQtPlanStagingSlots = 4;              // encodes whose parameters may be in flight at once

struct QtBatchArea {
    size_t off;              // bytes from the start of the store
    size_t elem;             // bytes per element
    size_t stride;           // elements per plane
    size_t count;            // elements in all = planes * stride
};

// The areas of the store.  The first four are what the caller may read (stable addresses).
enum QtArea {
    kQtLeaves,               // int32 [planes][Nr_min][leaf_ints]
    kQtNLeaves,              // int32 [planes]
    kQtParam,                // u32   [planes]: the threshold's bits or lambda in force
    kQtStats,                // u64   [planes][4]
    kQtSse,                  // u32   [planes][sum of Nr]
    kQtKeys,                 // u32   [planes][nkeys]
    kQtGains,                // i64   [planes][nkeys]
    kQtSelect,               // u64   [planes][kQtPlanSelectWords] (the unweighted select uses it as u32 [planes][kQtPlanSelectWords])
    kQtTopSum,               // u64   [planes]
    kQtCounts,               // int32 [planes][Ntop]
    kQtOffs,                 // int32 [planes][Ntop + 1]
    kQtRanks,                // u32   [planes]: the select's rank per plane, uploaded
    kQtValues,               // i64   [planes]: the weighted select's value per plane, uploaded
    kQtAreas
};

struct QtBatchPlan {
    int planes, nl, leaf_ints;
    int Nr[3];               // range blocks per plane of every level
    int Ntop, n1, nkeys, Nr_min;
    size_t sse_level[3];     // where the SSE of level l starts inside a plane's SSE row, in u32
    QtBatchArea a[kQtAreas]; // the areas, in the order they lie in
    size_t total;            // bytes of the store
    // The pinned staging buffer the per-plane parameters go up from: kQtPlanStagingSlots slots of `staging_slot` bytes, in each
    // u32 [planes] (param or ranks) at 0 and i64 [planes] (values) at staging_values
    size_t staging_values, staging_slot;
};

// 0 and *out, or -1 with *why naming the index that would pass 2^31 - 1 (or the argument that makes no plan)
inline int qt_batch_plan(int planes, int nl, const int* Nr, int leaf_ints, QtBatchPlan* out, const char** why)
{
    const char* dummy;
    if (!why) why = &dummy;
    *why = "";
    if (planes < 1 || planes > kQtPlanMaxPlanes) { *why = "planes (1 .. 65535: the plane is a grid dimension)"; return -1; }
    if (nl < 2 || nl > 3 || leaf_ints < 7 || leaf_ints > 9) { *why = "levels or leaf width"; return -1; }
    QtBatchPlan p{};
    p.planes = planes;
    p.nl = nl;
    p.leaf_ints = leaf_ints;
    size_t sum = 0;
    for (int l = 0; l < nl; l++) {
        if (Nr[l] < 1 || (l && (long long)Nr[l] != 4ll * Nr[l - 1])) { *why = "range blocks per level (each level has four times the blocks of the one above)"; return -1; }
        p.Nr[l] = Nr[l];
        p.sse_level[l] = sum;
        sum += (size_t)Nr[l];
    }
    p.Ntop = Nr[0];
    p.n1 = nl == 3 ? Nr[1] : 0;
    p.nkeys = p.Ntop + p.n1;
    p.Nr_min = Nr[nl - 1];
    const size_t P = (size_t)planes, lim = 0x7FFFFFFFull;
    size_t off = 0;
    bool ok = true;
    const char* bad = "";
    auto area = [&](int which, size_t elem, size_t stride, const char* name) {
        QtBatchArea& a = p.a[which];
        a.off = off;
        a.elem = elem;
        a.stride = stride;
        a.count = P * stride;                       // P < 2^16, stride < 2^35: no overflow of 64 bits
        if (a.count > lim && ok) { ok = false; bad = name; }
        off = (off + a.count * elem + 255) & ~(size_t)255;
    };
    area(kQtLeaves, 4, (size_t)p.Nr_min * (size_t)leaf_ints, "planes * Nr_min * kLeafInts (the leaf table)");
    area(kQtNLeaves, 4, 1, "planes");
    area(kQtParam, 4, 1, "planes");
    area(kQtStats, 8, 4, "planes * 4 (the statistics)");
    area(kQtSse, 4, sum, "planes * sum of Nr (the SSE store)");
    area(kQtKeys, 4, (size_t)p.nkeys, "planes * keys");
    area(kQtGains, 8, (size_t)p.nkeys, "planes * keys (the gains)");
    area(kQtSelect, 8, (size_t)kQtPlanSelectWords, "planes * select words");
    area(kQtTopSum, 8, 1, "planes");
    area(kQtCounts, 4, (size_t)p.Ntop, "planes * Ntop (the counts)");
    area(kQtOffs, 4, (size_t)p.Ntop + 1, "planes * (Ntop + 1) (the offsets)");
    area(kQtRanks, 4, 1, "planes");
    area(kQtValues, 8, 1, "planes");
    if (!ok) { *why = bad; return -1; }
    p.total = off;
    p.staging_values = (P * 4 + 255) & ~(size_t)255;
    p.staging_slot = p.staging_values + ((P * 8 + 255) & ~(size_t)255);
    *out = p;
    return 0;
}
