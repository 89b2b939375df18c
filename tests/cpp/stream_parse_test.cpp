// stream_parse_test.cpp -- the stream parsers of csrc/fic_stream.cpp under the host compiler's sanitizers.  Stand-alone: built
// from fic_stream.cpp alone (no HIP, no GPU) with -fsanitize=address,undefined (tests/test_stream_parse.py builds and runs it).
// One valid stream per tag, written by the library's own writers; the parser of the tag is then fed every prefix of it, every
// header int replaced by each of a list of hostile values, and a few hundred seeded replacements of one int of the body, at
// every zoom.  Each stream lies in a heap block of exactly its length, so a read past `len` is the sanitizer's to report.
// Every call must either return one of the documented codes, or a parsed structure whose sizes agree with its geometry.
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../fractal-image-compression_amd/csrc/fic_stream.h"

using namespace ficd;

namespace {

int g_calls = 0, g_parsed = 0, g_failures = 0;

#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            g_failures++;                                  \
            fprintf(stderr, "%s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);                  \
            fprintf(stderr, "\n");                         \
        }                                                  \
    } while (0)

uint32_t g_seed = 0xF1C0001u;
uint32_t rnd() { return g_seed = g_seed * 1664525u + 1013904223u; }
int rnd_below(int n) { return (int)((rnd() >> 8) % (uint32_t)n); }

const int kHostile[] = {0, 1, -1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 15, 16, 17, 24, 31, 32, 33, 40, 48, 64, 128, 255, 256, 4096, 32768, 46340,
                        46342, 65536, 1 << 20, 1 << 24, 1 << 28, 1 << 29, (1 << 30) - 16, 1 << 30, INT_MAX - 1, INT_MAX, INT_MIN, INT_MIN + 16,
                        -2, -4, -16};
const int kZooms[] = {1, 2, 4, 3, 0, -1};

bool documented(int rc) { return rc == FIC_E_GEOMETRY || rc == FIC_E_WINDOW || rc == FIC_E_ARGUMENT || rc == FIC_E_NOT_GREY; }

bool zoom_ok(int z) { return z == 1 || z == 2 || z == 4; }

// the parser of one tag on `len` bytes of its own heap block; returns its code after checking the contract
int parse(int tag, const std::vector<uint8_t>& bytes, size_t len, int zoom)
{
    uint8_t* heap = (uint8_t*)malloc(len ? len : 1);
    if (len) memcpy(heap, bytes.data(), len);
    g_calls++;
    int rc;
    if (tag == 0 || tag == 1 || tag == 4 || tag == 5) {
        const FixedFormat& F = tag == 0 ? kRunGrey : (tag == 1 ? kRunRgb : (tag == 4 ? kIsoGrey : kIsoRgb));
        FixedStream S;
        rc = parse_fixed(F, heap, (int64_t)len, zoom, &S);
        if (rc == FIC_OK) {
            g_parsed++;
            const FicGeom &g = S.g, &z = S.gz;
            const int per = F.QW + (F.iso ? 1 : 0);
            CHECK(zoom_ok(zoom), "tag %d: parsed at zoom %d", tag, zoom);
            CHECK(g.Nr > 0 && g.Nr == (g.W / g.B) * (g.H / g.B), "tag %d: Nr %d", tag, g.Nr);
            CHECK(S.rows.size() == (size_t)g.Nr * F.QW && S.iso.size() == (F.iso ? (size_t)g.Nr : 0), "tag %d: %zu row ints, %zu isometries for %d blocks",
                  tag, S.rows.size(), S.iso.size(), g.Nr);
            CHECK(z.W == zoom * g.W && z.H == zoom * g.H && z.B == zoom * g.B && z.Nr == g.Nr && z.Nd == g.Nd && z.wK == g.wK, "tag %d: zoomed geometry", tag);
            CHECK(F.exact ? (int64_t)len == 4 * (F.header_ints + (int64_t)per * g.Nr) : (int64_t)len >= 4 * (F.header_ints + (int64_t)per * g.Nr),
                  "tag %d: %zu bytes taken for %d blocks", tag, len, g.Nr);
            for (int j = 0; F.host_checked && j < g.Nr; j++)
                CHECK(S.rows[(size_t)F.QW * j] >= 0 && S.rows[(size_t)F.QW * j] < g.wK * g.wK && S.iso[j] >= 0 && S.iso[j] <= 7, "tag %d: row %d unchecked", tag, j);
        }
    } else {
        const QtFormat& F = tag == 2 ? kQtGreyStream : (tag == 3 ? kQtRgbStream : kQtRgbIsoStream);
        QtStream S;
        rc = parse_quadtree(F, heap, (int64_t)len, zoom, &S);
        if (rc == FIC_OK) {
            g_parsed++;
            CHECK(zoom_ok(zoom), "tag %d: parsed at zoom %d", tag, zoom);
            CHECK(S.L.nl >= 2 && S.L.nl <= kQtMaxLevels && S.Z.nl == S.L.nl, "tag %d: %d levels", tag, S.L.nl);
            long long pixels = 0, leaves = 0;
            for (int l = 0; l < S.L.nl && l < kQtMaxLevels; l++) {
                const FicGeom &g = S.L.g[l], &z = S.Z.g[l];
                CHECK(z.W == zoom * g.W && z.B == zoom * g.B && z.Nd == g.Nd && g.B == S.L.g[0].B >> l, "tag %d: level %d geometry", tag, l);
                CHECK(S.lv[l].size() % F.dev_ints == 0, "tag %d: level %d holds %zu ints", tag, l, S.lv[l].size());
                for (size_t i = 0; i + F.dev_ints <= S.lv[l].size(); i += F.dev_ints) {
                    const int32_t* e = &S.lv[l][i];
                    CHECK(e[0] >= 0 && e[0] + z.B <= z.W && e[1] >= 0 && e[1] + z.B <= z.H && e[0] % z.B == 0 && e[1] % z.B == 0, "tag %d: leaf at %d, %d", tag, e[0], e[1]);
                    CHECK(e[2] >= 0 && e[2] < z.Nd, "tag %d: domain block %d of %d", tag, e[2], z.Nd);
                    CHECK(e[3] >= 0 && (long long)e[3] + z.n <= (long long)z.W * z.H, "tag %d: sqbuf offset %d", tag, e[3]);
                    pixels += z.n;
                    leaves++;
                }
            }
            for (int l = S.L.nl; l < kQtMaxLevels; l++) CHECK(S.lv[l].empty(), "tag %d: leaves below the last level", tag);
            CHECK(pixels == (long long)S.Z.g[0].W * S.Z.g[0].H, "tag %d: the leaves cover %lld pixels", tag, pixels);
            const int per = 1 + F.QW + ((F.iso || (tag == 2 && S.L.g[0].n_iso == 8)) ? 1 : 0);
            CHECK((int64_t)len == 4 * (8 + per * leaves), "tag %d: %zu bytes taken for %lld leaves", tag, len, leaves);
        }
    }
    CHECK(rc == FIC_OK || (documented(rc) && fic_last_error_code() == rc && fic_last_error()[0]), "tag %d: code %d", tag, rc);
    free(heap);
    return rc;
}

void put(std::vector<uint8_t>& b, size_t i, int32_t v) { put_be32(b.data() + 4 * i, v); }

// 16 x 16, B = 4, wK = 2: 16 range blocks
std::vector<uint8_t> fixed_stream(int tag)
{
    const FixedFormat& F = tag == 0 ? kRunGrey : (tag == 1 ? kRunRgb : (tag == 4 ? kIsoGrey : kIsoRgb));
    const int Nr = 16;
    std::vector<int32_t> rows((size_t)Nr * F.QW), iso(Nr);
    for (int j = 0; j < Nr; j++) {
        rows[(size_t)F.QW * j] = rnd_below(4);
        for (int k = 1; k < F.QW; k++) rows[(size_t)F.QW * j + k] = (int)rnd() >> 8;
        iso[j] = j % 8;
    }
    std::vector<uint8_t> out(4 * (F.header_ints + (F.QW + 1) * (size_t)Nr));
    const int64_t n = write_fixed(F, rows.data(), F.iso ? iso.data() : nullptr, Nr, 16, 16, 4, 2, out.data(), (int64_t)out.size());
    CHECK(n > 0, "tag %d: writer gives %lld (%s)", tag, (long long)n, fic_last_error());
    out.resize(n > 0 ? (size_t)n : 0);
    return out;
}

// 32 x 32, levels 16..4, full search: a leaf of side 16, four of 8, a block split down to side 4, a leaf of side 16
std::vector<uint8_t> quadtree_stream(int tag)
{
    const QtFormat& F = tag == 2 ? kQtGreyStream : (tag == 3 ? kQtRgbStream : kQtRgbIsoStream);
    const int xyB[][3] = {{0, 0, 16}, {16, 0, 8}, {24, 0, 8}, {16, 8, 8}, {24, 8, 8}, {0, 16, 8}, {8, 16, 4}, {12, 16, 4}, {8, 20, 4}, {12, 20, 4},
                          {0, 24, 8}, {8, 24, 8}, {16, 16, 16}};
    const int n = (int)(sizeof(xyB) / sizeof(xyB[0]));
    std::vector<int32_t> leaves((size_t)n * F.leaf_ints);
    for (int i = 0; i < n; i++) {
        int32_t* e = &leaves[(size_t)i * F.leaf_ints];
        const int B = xyB[i][2], Dw = 2 * (32 / B) - 3;
        e[0] = xyB[i][0]; e[1] = xyB[i][1]; e[2] = B;
        e[3] = rnd_below(Dw * Dw);
        for (int k = 4; k < F.leaf_ints; k++) e[k] = (int)rnd() >> 8;
        if (tag != 3) e[F.leaf_ints - 1] = i % 8;
    }
    std::vector<uint8_t> out(4 * (8 + 8 * (size_t)n));
    const int64_t len = write_quadtree(F, leaves.data(), n, 32, 32, 16, 4, 0, tag == 3 ? 1 : 8, out.data(), (int64_t)out.size());
    CHECK(len > 0, "tag %d: writer gives %lld (%s)", tag, (long long)len, fic_last_error());
    out.resize(len > 0 ? (size_t)len : 0);
    return out;
}

void exercise(int tag)
{
    const bool fixed = tag == 0 || tag == 1 || tag == 4 || tag == 5;
    const std::vector<uint8_t> run = fixed ? fixed_stream(tag) : quadtree_stream(tag);
    const size_t header = fixed ? (tag < 2 ? 5 : 6) : 8, ints = run.size() / 4;
    for (int z : kZooms) {
        const int rc = parse(tag, run, run.size(), z);
        CHECK(zoom_ok(z) ? rc == FIC_OK : rc == FIC_E_ARGUMENT, "tag %d: the exact stream at zoom %d gives %d (%s)", tag, z, rc, fic_last_error());
    }
    for (size_t len = 0; len < run.size(); len++) {                 // every prefix: never the whole stream's result
        const int rc = parse(tag, run, len, 1 + (int)(len % 2));
        CHECK(rc == FIC_E_ARGUMENT, "tag %d: a prefix of %zu bytes gives %d", tag, len, rc);
    }
    std::vector<uint8_t> longer(run);                               // trailing bytes: only the .run readers take them
    longer.resize(run.size() + 4);
    CHECK(parse(tag, longer, longer.size(), 1) == (tag < 2 ? FIC_OK : FIC_E_ARGUMENT), "tag %d: trailing bytes", tag);
    for (size_t i = 0; i < header; i++)                             // every header int, every hostile value, every zoom
        for (int v : kHostile)
            for (int z : kZooms) {
                std::vector<uint8_t> bad(run);
                put(bad, i, v);
                parse(tag, bad, bad.size(), z);
            }
    for (int k = 0; k < 400; k++) {                                 // one int of the body
        std::vector<uint8_t> bad(run);
        const int v = (k % 3) ? kHostile[rnd_below((int)(sizeof(kHostile) / sizeof(kHostile[0])))] : (int)rnd();
        put(bad, header + (size_t)rnd_below((int)(ints - header)), v);
        parse(tag, bad, bad.size(), kZooms[k % 3]);
    }
    // two header ints at once: a hostile image size beside a hostile block side / level / leaf count
    for (int a : kHostile)
        for (int b : kHostile) {
            std::vector<uint8_t> bad(run);
            put(bad, 1, a);
            put(bad, 2, a);
            put(bad, header - 1, b);
            parse(tag, bad, bad.size(), 4);
            put(bad, header - 2, b);
            parse(tag, bad, bad.size(), 4);
        }
}

}  // namespace

int main()
{
    for (int tag : {0, 1, 4, 5, 2, 3, 6}) exercise(tag);
    printf("%d parser calls, %d parsed, %d failures\n", g_calls, g_parsed, g_failures);
    return g_failures ? 1 : 0;
}
