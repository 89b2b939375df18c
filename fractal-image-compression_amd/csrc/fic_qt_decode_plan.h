// fic_qt_decode_plan.h -- the decode side of a batched quadtree context (fic_qt_ctx_decode_zoom_host / _collage_host,
// fic_capi_qt_ctx.cpp): where a leaf's squares lie in the decoder's `sqbuf`, as a closed form of the leaf's
// position (k_qt_resolve, fic_quadtree.hip, evaluates it per leaf, so no scan runs over the table), and where the areas of the
// decode workspace lie in its one device store.  Plain C++ without HIP, integers in and out; tests/cpp/qt_decode_plan_test.cpp
// runs it under the address and undefined-behaviour sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define FIC_QT_PLAN_FN __host__ __device__ inline
#else
#define FIC_QT_PLAN_FN inline
#endif

// The decoder visits the leaves in the table's order -- top blocks in scanline order, children TL, TR, BL, BR depth first -- and
// a leaf's pixels row by row; the squares of an iteration lie in `sqbuf` in that order, because Java's float accumulation of them
// depends on it.  The offset of the leaf {x, y, B} of an image of Rw_top top blocks per row is therefore the
// number of pixels of the leaves before it: the t = (y / B_max) Rw_top + x / B_max top blocks before its own, and inside that one,
// at every side s from B_max / 2 down to B, the quadrants before the one the leaf lies in: 2 [yr & s] + [xr & s] of them, s^2
// pixels each, whatever they are split into (xr = x mod B_max, yr = y mod B_max).  At zoom z every side grows z-fold.
// Precondition: B_max a power of two, B a power of two with B <= B_max, x and y non-negative multiples of B.
FIC_QT_PLAN_FN long long qt_decode_sqoff(int x, int y, int B, int B_max, int Rw_top, int zoom)
{
    const int xr = x & (B_max - 1), yr = y & (B_max - 1);
    long long px = ((long long)(y / B_max) * Rw_top + x / B_max) * B_max * B_max;
    for (int s = B_max / 2; s >= B; s /= 2) px += (long long)s * s * (2 * ((yr & s) != 0) + ((xr & s) != 0));
    return px * zoom * zoom;
}

// One resolved leaf, as k_qt_resolve writes it and k_qt_paint_planes reads it: kQtEntryInts int32.  The first words are the
// words of the stream decoder's leaf (FicQtLeaf / FicQtLeafIso, fic_launch.h) at the decode's zoom.
enum QtEntryWord {
    kQtEntryX, kQtEntryY,    // the leaf's top-left pixel, times zoom
    kQtEntryGi,              // global domain block (window_to_global of the leaf's level)
    kQtEntrySqoff,           // qt_decode_sqoff
    kQtEntryQ,               // the quantised row behind idx_local, 4 words: {qa, qb, iso, 0} grey, {q1, q2, q3, q4} colour
    kQtEntryIso = 8,
    kQtEntrySide,            // B times zoom
    kQtEntryInts = 12        // 48 bytes: three 16-byte loads (the last two words are 0)
};

// The areas of the decode store, each at a multiple of 256 bytes behind the one before it.  The loop's own areas (the last three)
// are used by a decode at zoom 1; a zoomed decode takes them, at the zoomed size, from a decode job's arena.
enum QtDecodeArea {
    kQtDecEntries,           // int32 [planes][Nr_min][kQtEntryInts]
    kQtDecCells,             // int32 [planes][Nr_min]: the leaf that covers every cell of side B_min, -1 before the resolve
    kQtDecCover,             // int32 [planes]: cells claimed by the plane's leaves (Nr_min for a table that tiles the image)
    kQtDecImage,             // pixels [planes][H][W]: the decode at zoom 1, the collage
    kQtDecState,             // FicDecodeState [planes]
    kQtDecScaled,            // pixels [planes][H / 2][W / 2]
    kQtDecSq,                // u32 [sq_words]: the squares and the float sum's scratch (fic_decode_sq_words)
    kQtDecAreas
};

struct QtDecodeArea1 {
    size_t off, bytes;
};

struct QtDecodePlan {
    int planes, Nr_min;
    QtDecodeArea1 a[kQtDecAreas];
    size_t total;            // bytes of the store
};

// 0 and *out, or -1 with *why naming the index that would pass 2^31 - 1 (or the argument that makes no plan).  w, h: the
// image; px_bytes 1 (grey) or 4 (packed ARGB); max_zoom: the largest zoom the decode runs at -- a pixel of a plane and its
// square's place in `sqbuf` (an int32 of the entries) are indices below max_zoom^2 w h, whatever the number of planes (the
// kernels add the plane in 64 bits); state_bytes: sizeof(FicDecodeState); sq_words: fic_decode_sq_words(planes, w h).  The
// offsets do not depend on max_zoom.
inline int qt_decode_plan(int planes, int w, int h, int B_min, int px_bytes, int max_zoom, size_t state_bytes, size_t sq_words, QtDecodePlan* out,
                          const char** why)
{
    const char* dummy;
    if (!why) why = &dummy;
    *why = "";
    if (planes < 1 || planes > 65535) { *why = "planes (1 .. 65535: the plane is a grid dimension)"; return -1; }
    if (w < 1 || h < 1 || B_min < 4 || (w % B_min) || (h % B_min) || (px_bytes != 1 && px_bytes != 4) || max_zoom < 1) { *why = "image, B_min, pixel or zoom"; return -1; }
    const size_t lim = 0x7FFFFFFFull, P = (size_t)planes, npix = (size_t)w * (size_t)h, nr = (size_t)(w / B_min) * (size_t)(h / B_min);
    if (npix * (size_t)max_zoom * (size_t)max_zoom > lim) { *why = "zoom^2 * w * h (a plane's pixels)"; return -1; }
    if (P * nr * kQtEntryInts > lim) { *why = "planes * Nr_min * kQtEntryInts (the resolved leaves)"; return -1; }
    QtDecodePlan p{};
    p.planes = planes;
    p.Nr_min = (int)nr;
    size_t off = 0;
    auto area = [&](int which, size_t bytes) {
        p.a[which].off = off;
        p.a[which].bytes = bytes;
        off = (off + bytes + 255) & ~(size_t)255;
    };
    area(kQtDecEntries, P * nr * kQtEntryInts * 4);
    area(kQtDecCells, P * nr * 4);
    area(kQtDecCover, P * 4);
    area(kQtDecImage, P * npix * (size_t)px_bytes);
    area(kQtDecState, P * state_bytes);
    area(kQtDecScaled, P * (size_t)(w / 2) * (size_t)(h / 2) * (size_t)px_bytes);
    area(kQtDecSq, sq_words * 4);
    p.total = off;
    *out = p;
    return 0;
}
