// csrc/fic_qt_batch_plan.h as a program of its own, built with the host compiler's address and undefined-behaviour sanitizers
// (tests/test_qt_batch_plan.py): for the geometries of the batched quadtree tests, every area of a context's store starts at a
// multiple of 256 bytes, no two overlap, the strides are those the kernels are given, the total is the end of the last area,
// and a plan whose element indices would pass 2^31 - 1 is refused (and only such a plan).
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../fractal-image-compression_amd/csrc/fic_qt_batch_plan.h"

static int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            failures++;                                   \
            printf("FAIL %s:%d: ", __FILE__, __LINE__);   \
            printf(__VA_ARGS__);                          \
            printf("\n");                                 \
        }                                                 \
    } while (0)

struct Geo {
    int w, h, B_max, B_min;
};

static int levels(const Geo& g, int* Nr)
{
    int nl = 0;
    for (int B = g.B_max; B >= g.B_min; B /= 2) Nr[nl++] = (g.w / B) * (g.h / B);
    return nl;
}

static void check_plan(const Geo& g, int planes, int leaf_ints)
{
    int Nr[3] = {0, 0, 0};
    const int nl = levels(g, Nr);
    QtBatchPlan p;
    memset(&p, 0xAB, sizeof(p));
    const char* why = nullptr;
    const int rc = qt_batch_plan(planes, nl, Nr, leaf_ints, &p, &why);
    CHECK(rc == 0, "%dx%d %d->%d planes %d: refused: %s", g.w, g.h, g.B_max, g.B_min, planes, why);
    if (rc) return;
    const size_t P = (size_t)planes;
    size_t sum = 0;
    for (int l = 0; l < nl; l++) {
        CHECK(p.Nr[l] == Nr[l] && p.sse_level[l] == sum, "level %d: Nr %d, SSE offset %zu, want %d / %zu", l, p.Nr[l], p.sse_level[l], Nr[l], sum);
        sum += (size_t)Nr[l];
    }
    const int n1 = nl == 3 ? Nr[1] : 0;
    CHECK(p.planes == planes && p.nl == nl && p.leaf_ints == leaf_ints && p.Ntop == Nr[0] && p.n1 == n1 && p.nkeys == Nr[0] + n1 && p.Nr_min == Nr[nl - 1],
          "the plan's counts");
    // the strides the kernels are given, the element sizes of what lies there
    const size_t stride[kQtAreas] = {(size_t)Nr[nl - 1] * leaf_ints, 1, 1, 4, sum, (size_t)Nr[0] + n1, (size_t)Nr[0] + n1, (size_t)kQtPlanSelectWords, 1,
                                     (size_t)Nr[0], (size_t)Nr[0] + 1, 1, 1};
    const size_t elem[kQtAreas] = {4, 4, 4, 8, 4, 4, 8, 8, 8, 4, 4, 4, 8};
    size_t end = 0;
    for (int i = 0; i < kQtAreas; i++) {
        const QtBatchArea& a = p.a[i];
        CHECK(a.stride == stride[i] && a.elem == elem[i] && a.count == P * stride[i], "area %d: stride %zu elem %zu count %zu", i, a.stride, a.elem, a.count);
        CHECK(a.off % 256 == 0, "area %d starts at %zu: not a multiple of 256", i, a.off);
        CHECK(a.off >= end, "area %d starts at %zu, inside the area before it (ends at %zu)", i, a.off, end);
        CHECK(a.count <= 0x7FFFFFFFull, "area %d: %zu elements", i, a.count);
        end = a.off + a.count * a.elem;
    }
    CHECK(p.total >= end && p.total - end < 256 && p.total % 256 == 0, "total %zu, the last area ends at %zu", p.total, end);
    // the select area serves the unweighted select as u32 [planes][words] as well
    CHECK(P * kQtPlanSelectWords * 4 <= p.a[kQtSelect].count * p.a[kQtSelect].elem, "the select area as u32");
    // the three host results lie one behind the other: one copy fetches them
    const size_t words = (P * 4 + 255) & ~(size_t)255;
    CHECK(p.a[kQtParam].off == p.a[kQtNLeaves].off + words && p.a[kQtStats].off == p.a[kQtParam].off + words, "n_leaves, param, stats are neighbours");
    CHECK(p.staging_values % 256 == 0 && p.staging_values >= P * 4 && p.staging_slot % 256 == 0 && p.staging_slot >= p.staging_values + P * 8,
          "staging: values at %zu, slot %zu", p.staging_values, p.staging_slot);
    // every byte of the store belongs to at most one area: paint them
    if (p.total <= (size_t)64 << 20) {
        std::vector<unsigned char> owner(p.total, 0xFF);
        for (int i = 0; i < kQtAreas; i++)
            for (size_t b = p.a[i].off; b < p.a[i].off + p.a[i].count * p.a[i].elem; b++) {
                if (owner[b] != 0xFF) { CHECK(false, "byte %zu belongs to areas %d and %d", b, owner[b], i); break; }
                owner[b] = (unsigned char)i;
            }
    }
}

static void check_refused(const Geo& g, int planes, int leaf_ints, const char* part)
{
    int Nr[3] = {0, 0, 0};
    const int nl = levels(g, Nr);
    QtBatchPlan p;
    memset(&p, 0x5C, sizeof(p));
    const QtBatchPlan before = p;
    const char* why = nullptr;
    const int rc = qt_batch_plan(planes, nl, Nr, leaf_ints, &p, &why);
    CHECK(rc != 0, "%dx%d %d->%d planes %d: accepted", g.w, g.h, g.B_max, g.B_min, planes);
    CHECK(why && strstr(why, part), "%dx%d planes %d: refused for '%s', want '%s'", g.w, g.h, planes, why ? why : "(null)", part);
    CHECK(memcmp(&p, &before, sizeof(p)) == 0, "a refused plan was written");
}

int main()
{
    const Geo geos[] = {{32, 32, 16, 4}, {32, 32, 8, 4}, {64, 48, 16, 4}, {272, 272, 16, 4}, {256, 256, 16, 8}, {512, 512, 16, 4}};
    int plans = 0;
    for (const Geo& g : geos)
        for (int planes : {1, 3, 16, 64})
            for (int leaf_ints : {7, 9}) {
                check_plan(g, planes, leaf_ints);
                plans++;
            }
    // the 2^31 limits: 1024 x 1024, 16 -> 4 has 65536 blocks of side 4, 458752 leaf ints per plane at 7 ints a row
    const Geo big{1024, 1024, 16, 4};
    check_plan(big, 4681, 7);               // 4681 * 458752 = 2147418112 <= 2^31 - 1
    check_refused(big, 4682, 7, "leaf table");
    check_plan(big, 3640, 9);               // 3640 * 589824 = 2146959360
    check_refused(big, 3641, 9, "leaf table");
    check_plan(geos[0], 65535, 9);          // the most planes a grid takes
    check_refused(geos[0], 65536, 9, "planes");
    check_refused(geos[0], 0, 7, "planes");
    check_refused(geos[0], -1, 7, "planes");
    check_refused(geos[3], 65535, 9, "leaf table");      // 65535 * 4624 * 9
    check_refused(geos[0], 1, 6, "leaf width");
    {
        int Nr[3] = {4, 16, 65};            // not a ladder
        QtBatchPlan p;
        const char* why = nullptr;
        CHECK(qt_batch_plan(1, 3, Nr, 7, &p, &why) != 0 && strstr(why, "four times"), "a ladder that is none");
    }
    printf("%d plans checked\n%d failures\n", plans + 3, failures);
    return failures ? 1 : 0;
}
