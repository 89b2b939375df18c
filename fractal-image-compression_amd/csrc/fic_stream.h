// fic_stream.h -- the stream formats (fic_stream.cpp): every tag's writer, and its reader as a parser from bytes to a plain
// host structure that the decoders (fic_capi_decode.cpp, fic_capi_quadtree.cpp) take.  With them the host code they stand on:
// the calling thread's error state, the geometry of an image and of a zoomed decode, big-endian ints, the quadtree's levels.
// No HIP: this header and fic_stream.cpp build with the plain host compiler (tests/cpp/stream_parse_test.cpp).
//   tag 0 / 1   .run, grey / colour        {isRGB, w, h, B, wK}                       rows {idx_local, qa, qb} / {idx_local, q1..q4}
//   tag 4 / 5   the same + isometries      {tag, w, h, 0, B, wK}                      rows {row, iso}                    
//   tag 2       grey quadtree              {2, w, h, B_max, B_min, wK, n_iso, n}      rows {B, idx_local, qa, qb[, iso]} (4.13)
//   tag 3 / 6   colour quadtree [+ iso]    {tag, w, h, 0, B_max, B_min, wK, n}        rows {B, idx_local, q1..q4[, iso]} (4.14, 4.17)
#pragma once
#include <stdint.h>
#include <string>
#include <vector>

#include "../../include/fic.h"
#include "fic_device.h"

namespace ficd {

// message + code of the last failure on the calling thread (fic_last_error / fic_last_error_code)
extern thread_local std::string g_err;
extern thread_local int g_err_code;
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

// Geometry as the reference derives it (FC:111-116, FC:1019-1022) + what it needs to not throw; out == nullptr: validate only
int make_geometry(int w, int h, int B, int wK, int n_iso, int planes, FicGeom* out);
// Decoders only: the geometry (zoom w, zoom h, zoom B, wK) of a decode at zoom 1, 2 or 4 of a stream whose own geometry
// (w, h, B, wK) make_geometry accepts; block sides up to 64.  FIC_E_ARGUMENT for another zoom.
int make_decode_geometry(int w, int h, int B, int wK, int n_iso, int planes, int zoom, FicGeom* out);

// DataOutputStream.writeInt / DataInputStream.readInt of the .run streams (FC:234-256, 372-374): big-endian int32
inline void put_be32(uint8_t* p, int32_t v)
{
    uint32_t u = (uint32_t)v;
    p[0] = (uint8_t)(u >> 24); p[1] = (uint8_t)(u >> 16); p[2] = (uint8_t)(u >> 8); p[3] = (uint8_t)u;
}
inline int32_t get_be32(const uint8_t* p)
{
    return (int32_t)(((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3]);
}

// ---- fixed block size: tags 0, 1, 4, 5 ------------------------------------------------------------------------------------------
struct FixedFormat {
    int tag;                 // the first header int; tag 1 stands for any isRGB != 0 (FC:548)
    int header_ints;         // 5 {isRGB, w, h, B, wK}; 6 {tag, w, h, 0, B, wK}: the 0 where a .run holds B, so no older reader takes it
    int QW;                  // ints of a quantised row: 3 grey {idx_local, qa, qb}, 5 colour {idx_local, q1, q2, q3, q4}
    bool iso;                // an isometry 0..7 behind every row
    bool exact;              // the reader takes exactly the stream's length; false: at least (trailing bytes are never read, FC:372-374)
    bool host_checked;       // the writer checks the geometry, the row count and the isometries, the reader every idx_local and
                             // isometry; false: any n_ranges is written, and a row outside the window is the paint kernel's to flag
    const char *writer, *reader;
};
//                                      tag hdr QW iso    exact  checked
inline constexpr FixedFormat kRunGrey{0, 5, 3, false, false, false, "fic_write_run_gray", "fic_decode_gray_run"},
                             kRunRgb{1, 5, 5, false, false, false, "fic_write_run_rgb", "fic_decode_rgb_run"},
                             kIsoGrey{4, 6, 3, true, true, true, "fic_write_run_gray_iso", "fic_decode_gray_iso_run"},
                             kIsoRgb{5, 6, 5, true, true, true, "fic_write_run_rgb_iso", "fic_decode_rgb_iso_run"};

struct FixedStream {
    FicGeom g{}, gz{};       // the stream's geometry and the one the decode runs on
    bool sized = false;      // gz is valid: the size the decoder reports, which a .run reader knows before a parse fails on the body
    std::vector<int32_t> rows, iso;   // [g.Nr][QW], [g.Nr] (empty without a column)
};
// iso == NULL exactly for the formats without a column
int64_t write_fixed(const FixedFormat& F, const int32_t* rows, const int32_t* iso, int n_ranges, int w, int h, int B, int wK,
                    uint8_t* out, int64_t capacity);
int parse_fixed(const FixedFormat& F, const uint8_t* run, int64_t len, int zoom, FixedStream* out);

// ---- quadtree: tags 2, 3, 6 -----------------------------------------------------------------------------------------------------
constexpr int kQtMaxLevels = 3;   // 16 -> 8 -> 4
// The levels B_max, B_max / 2, ..., B_min and their geometries (wK = 0: full search at every level, wK_B = Dw_B).
struct QtLevels {
    int nl = 0;
    FicGeom g[kQtMaxLevels];
};
int qt_levels(int w, int h, int B_max, int B_min, int wK, int n_iso, QtLevels* L);

struct QtFormat {
    int tag;
    int QW;                  // ints of a quantised row, as above
    bool iso;                // every row ends with an isometry 0..7 (tag 6); a tag-2 row does when the header's n_iso is 8
    int leaf_ints;           // a leaf of the encoder's table: {x, y, B, row[, iso]} (QtGrey / QtRgb / QtRgbIso::kLeafInts, fic_launch.h)
    int dev_ints;            // a leaf of the decoder's per-level lists (FicQtLeaf / FicQtLeafIso, fic_launch.h), in ints
    const char *kind, *writer, *reader;
};
//                                            tag QW iso  leaf dev
inline constexpr QtFormat kQtGreyStream{2, 3, false, 7, 8, "quadtree", "fic_write_run_quadtree", "fic_decode_quadtree_run"},
                          kQtRgbStream{3, 5, false, 8, 8, "colour quadtree", "fic_write_run_rgb_quadtree", "fic_decode_rgb_quadtree_run"},
                          kQtRgbIsoStream{6, 5, true, 9, 9, "colour quadtree (isometries)", "fic_write_run_rgb_quadtree_iso",
                                          "fic_decode_rgb_quadtree_iso_run"};

struct QtStream {
    QtLevels L, Z;           // the stream's levels and the same at `zoom`, where the paint runs
    // per level its leaves in stream order, dev_ints each: {zoom x, zoom y, global domain block, offset of the leaf's squares in
    // sqbuf, q[4]: {qa, qb, iso, 0} grey / {q1, q2, q3, q4} colour[, iso]} -- the words of FicQtLeaf / FicQtLeafIso
    std::vector<int32_t> lv[kQtMaxLevels];
};
int64_t write_quadtree(const QtFormat& F, const int32_t* leaves, int n_leaves, int w, int h, int B_max, int B_min, int wK, int n_iso,
                       uint8_t* out, int64_t capacity);
int parse_quadtree(const QtFormat& F, const uint8_t* run, int64_t len, int zoom, QtStream* out);

}  // namespace ficd
