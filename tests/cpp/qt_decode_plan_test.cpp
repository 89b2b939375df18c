// csrc/fic_qt_decode_plan.h as a program of its own, built with the host compiler's address and undefined-behaviour sanitizers
// (tests/test_qt_decode_plan.py).  The layout of the decode store: every area at a multiple of 256 bytes, none overlapping, the
// sizes the kernels index, the total the end of the last one, and the refusal of what would pass 2^31 - 1.  The closed form
// qt_decode_sqoff against the running sum of a plain walk in the stream parser's order (top blocks in scanline order, children
// TL, TR, BL, BR depth first, zoom^2 B^2 squares per leaf): every tree of one top block on the ladders 16 -> 4, 16 -> 8 and
// 8 -> 4, and random trees on the shapes of tests/test_gpu_quadtree_batch_decode.py, at zoom 1, 2 and 4.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../fractal-image-compression_amd/csrc/fic_qt_decode_plan.h"

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

constexpr size_t kStateBytes = 424;      // sizeof(FicDecodeState); any size serves the layout

static void check_plan(const Geo& g, int planes, int px, int zoom)
{
    const size_t P = (size_t)planes, npix = (size_t)g.w * g.h, nr = (size_t)(g.w / g.B_min) * (g.h / g.B_min);
    const size_t sq_words = P * (npix + 1234);
    QtDecodePlan p;
    memset(&p, 0xAB, sizeof(p));
    const char* why = nullptr;
    const int rc = qt_decode_plan(planes, g.w, g.h, g.B_min, px, zoom, kStateBytes, sq_words, &p, &why);
    CHECK(rc == 0, "%dx%d planes %d zoom %d: refused: %s", g.w, g.h, planes, zoom, why);
    if (rc) return;
    CHECK(p.planes == planes && p.Nr_min == (int)nr, "the plan's counts");
    const size_t bytes[kQtDecAreas] = {P * nr * kQtEntryInts * 4, P * nr * 4, P * 4, P * npix * px, P * kStateBytes, P * (npix / 4) * px, sq_words * 4};
    size_t end = 0;
    for (int i = 0; i < kQtDecAreas; i++) {
        CHECK(p.a[i].bytes == bytes[i], "area %d: %zu bytes, want %zu", i, p.a[i].bytes, bytes[i]);
        CHECK(p.a[i].off % 256 == 0, "area %d starts at %zu: not a multiple of 256", i, p.a[i].off);
        CHECK(p.a[i].off >= end, "area %d starts at %zu, inside the area before it (ends at %zu)", i, p.a[i].off, end);
        end = p.a[i].off + p.a[i].bytes;
    }
    CHECK(p.total >= end && p.total - end < 256 && p.total % 256 == 0, "total %zu, the last area ends at %zu", p.total, end);
    // the offsets do not depend on the zoom: a store made for one decode serves every later one
    QtDecodePlan q;
    CHECK(qt_decode_plan(planes, g.w, g.h, g.B_min, px, 1, kStateBytes, sq_words, &q, &why) == 0 && memcmp(&p, &q, sizeof(p)) == 0, "the plan at zoom 1");
}

static void check_refused(const Geo& g, int planes, int px, int zoom, const char* part)
{
    QtDecodePlan p;
    memset(&p, 0x5C, sizeof(p));
    const QtDecodePlan before = p;
    const char* why = nullptr;
    const int rc = qt_decode_plan(planes, g.w, g.h, g.B_min, px, zoom, kStateBytes, 16, &p, &why);
    CHECK(rc != 0, "%dx%d planes %d zoom %d: accepted", g.w, g.h, planes, zoom);
    CHECK(why && strstr(why, part), "%dx%d planes %d: refused for '%s', want '%s'", g.w, g.h, planes, why ? why : "(null)", part);
    CHECK(memcmp(&p, &before, sizeof(p)) == 0, "a refused plan was written");
}

// The parser's walk (qt_tile, fic_stream.cpp).  split[t]: bit 4 the top block t splits, bit c (0..3) its child c does.
struct Walk {
    Geo g;
    int zoom;
    const std::vector<int>* split;
    long long run = 0;
    int leaves = 0;
    void visit(int t, int x, int y, int B, int child)
    {
        const int s = (*split)[t];
        const bool top = B == g.B_max;
        const bool splits = B > g.B_min && (top ? (s & 16) != 0 : (s & (1 << child)) != 0);
        if (!splits) {
            const long long got = qt_decode_sqoff(x, y, B, g.B_max, g.w / g.B_max, zoom);
            CHECK(got == run, "%dx%d %d->%d zoom %d: leaf (%d, %d, %d): sqoff %lld, the walk has %lld", g.w, g.h, g.B_max, g.B_min, zoom, x, y, B, got, run);
            run += (long long)zoom * zoom * B * B;
            leaves++;
            return;
        }
        const int hb = B / 2;
        const int dx[4] = {0, hb, 0, hb}, dy[4] = {0, 0, hb, hb};
        for (int c = 0; c < 4; c++) visit(t, x + dx[c], y + dy[c], hb, top ? c : child);
    }
    void all()
    {
        int t = 0;
        for (int y = 0; y < g.h; y += g.B_max)
            for (int x = 0; x < g.w; x += g.B_max) visit(t++, x, y, g.B_max, 0);
        CHECK(run == (long long)zoom * zoom * g.w * g.h, "the walk covers %lld pixels", run);
    }
};

int main()
{
    const Geo shapes[] = {{32, 32, 16, 4}, {32, 32, 8, 4}, {64, 48, 16, 4}, {272, 272, 16, 4}};
    int plans = 0;
    for (const Geo& g : shapes)
        for (int planes : {1, 3, 64})
            for (int px : {1, 4})
                for (int zoom : {1, 2, 4}) {
                    check_plan(g, planes, px, zoom);
                    plans++;
                }
    check_plan(Geo{512, 512, 16, 4}, 64, 1, 4);
    check_plan(Geo{32, 32, 16, 4}, 65535, 4, 1);
    check_refused(shapes[0], 0, 1, 1, "planes");
    check_refused(shapes[0], 65536, 1, 1, "planes");
    check_refused(shapes[0], 1, 2, 1, "pixel");
    check_refused(Geo{30, 32, 16, 4}, 1, 1, 1, "image");
    check_refused(Geo{16384, 16384, 16, 4}, 1, 1, 4, "zoom^2");               // 2^28 pixels: zoom 2 fits, zoom 4 is 2^32
    check_plan(Geo{16384, 16384, 16, 8}, 1, 1, 2);
    check_refused(Geo{2048, 2048, 16, 4}, 1024, 1, 1, "resolved leaves");     // 1024 * 262144 * 12 ints

    int trees = 0, total_leaves = 0;
    // every tree of one top block
    const Geo one[] = {{16, 16, 16, 4}, {16, 16, 16, 8}, {8, 8, 8, 4}};
    for (const Geo& g : one)
        for (int zoom : {1, 2, 4}) {
            const bool three = g.B_max / g.B_min == 4;
            for (int s = 0; s < (three ? 32 : 17); s++) {
                if (s < 16 && s != 0) continue;            // children only under a root that splits; s = 0: the one leaf
                if (!three && (s & 15)) continue;
                std::vector<int> split{s};
                Walk w{g, zoom, &split};
                w.all();
                trees++;
                total_leaves += w.leaves;
            }
        }
    // random trees on the test shapes (a fixed linear congruential sequence)
    unsigned long long seed = 88172645463325252ull;
    for (const Geo& g : shapes)
        for (int zoom : {1, 2, 4})
            for (int rep = 0; rep < 20; rep++) {
                std::vector<int> split((size_t)(g.w / g.B_max) * (g.h / g.B_max));
                for (int& s : split) {
                    seed = seed * 6364136223846793005ull + 1442695040888963407ull;
                    s = (int)((seed >> 33) & 31);
                    if (rep == 0) s = 0;                   // the two extremes once each
                    if (rep == 1) s = 31;
                }
                Walk w{g, zoom, &split};
                w.all();
                trees++;
                total_leaves += w.leaves;
            }
    printf("%d plans checked\n%d trees walked, %d leaves\n%d failures\n", plans, trees, total_leaves, failures);
    return failures ? 1 : 0;
}
