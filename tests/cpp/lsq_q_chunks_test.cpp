// lsq_q_chunks_test.cpp -- stand-alone host check of the pool-chunk arithmetic of the two matrix-core least-squares sweeps
// (csrc/fic_lsq_q_chunks.h, DESIGN.md sections 4.21 and 4.22): over (N_d, requested chunks, B, n_iso, columns, planes) from
// N_d = 1 up to the pools of 4096 x 4096 images it checks, for the joint-RGB plan and for the grey plan, that no chunk is empty,
// that the chunks cover every domain tile exactly once and in order, and that the launchers' predicate holds; for RGB also that
// the slot count is the chunk count, that the count never exceeds what was asked for (nor the launcher's limit), that the largest
// candidate a chunk can write fits the 32 bits of the per-lane minima beside their "none" value, and that pools past that cap are
// refused; for grey that no chunk is longer than the 22-bit candidate field allows.  Given the recorded table
// tests/golden/lsq_q_chunks.txt as its argument it compares both plans with it row by row.  Built by
// tests/test_rgb_lsq_q_bound.py with the host compiler and its sanitizers; never runs on a GPU.
#include <stdint.h>
#include <stdio.h>

#include "../../fractal-image-compression_amd/csrc/fic_lsq_q_chunks.h"

static long long failures = 0, plans = 0, grey_plans = 0;
static const char* who = "rgb";               // the plan under check, for the messages

static void fail(const char* what, long long Nd, long long columns, int B, int n_iso, int planes, long long req)
{
    if (failures < 20) printf("FAIL %s %s: Nd=%lld columns=%lld B=%d n_iso=%d planes=%d requested=%lld\n", who, what, Nd, columns, B, n_iso, planes, req);
    failures++;
}

// column tiles one wave of k_sweep_lsq_q keeps (fic_lsq_q.hip's lsq_q_ctw)
static int grey_ctw(int B) { return B == 4 ? 8 : (B == 8 ? 4 : 2); }

// what both plans owe the kernels: the launchers' predicate, then coverage, in order, nothing empty
#define FAIL(what) fail(what, Nd, columns, B, n_iso, planes, req)
static void check_cut(int tiles_per_chunk, int nchunks, long long Nd, long long columns, int B, int n_iso, int planes, long long req)
{
    const long long ndtiles = (Nd + 31) / 32;
    if (nchunks < 1 || tiles_per_chunk < 1) return FAIL("counts");
    if (nchunks > ndtiles) FAIL("too many chunks");
    // the launchers' conditions, as the launchers state them and written out
    const bool cover = (long long)tiles_per_chunk * (nchunks - 1) < ndtiles && (long long)tiles_per_chunk * nchunks >= ndtiles;
    if (!cover || !lsq_q_chunks_cover(ndtiles, tiles_per_chunk, nchunks)) FAIL("launcher");
    if (lsq_q_chunks_cover(ndtiles, tiles_per_chunk, nchunks + 1) || lsq_q_chunks_cover(ndtiles, tiles_per_chunk, nchunks - 1) ||
        lsq_q_chunks_cover(ndtiles, 0, nchunks))
        FAIL("predicate accepts a wrong count");
    // walk the chunks as the kernel does (all of a small plan; both ends of a large one, whose middle follows from the launcher's
    // conditions above: chunk c starts at c * tiles_per_chunk and is full)
    for (int part = 0; part < 2; part++) {
        const int c0 = part == 0 ? 0 : (nchunks > 4096 ? nchunks - 2048 : nchunks);
        const int c1 = part == 0 ? (nchunks > 4096 ? 2048 : nchunks) : nchunks;
        long long next = (long long)c0 * tiles_per_chunk;
        for (int c = c0; c < c1; c++) {
            int t0, t1;
            lsq_q_chunk_tiles((int)ndtiles, tiles_per_chunk, c, &t0, &t1);
            if (t1 <= t0) FAIL("empty chunk");
            if (t0 != next) FAIL("gap or overlap");
            if (t1 > ndtiles) FAIL("past the pool");
            if ((long long)t0 * 32 >= Nd) FAIL("chunk without a real row");   // its slot is written
            next = t1;
            if (c == nchunks - 1 && t1 != ndtiles) FAIL("tail not covered");
        }
    }
}

static void check(long long Nd, long long columns, int B, int n_iso, int planes, long long req)
{
    const LsqRgbQPlan p = lsq_rgb_q_plan(Nd, columns, B, n_iso, planes, req);
    plans++;
    if (!p.ok) return FAIL("refused");
    const long long ndtiles = (Nd + 31) / 32;
    if (p.ndtiles != ndtiles) FAIL("ndtiles");
    if (p.nchunks < 1 || p.tiles_per_chunk < 1) return FAIL("counts");
    if (p.nslots != p.nchunks) FAIL("slots");
    if (p.nchunks > FIC_LSQ_RGB_Q_MAX_CHUNKS || p.nchunks > ndtiles) FAIL("too many chunks");
    if (req > 0 && p.nchunks > req) FAIL("more chunks than requested");
    if (req == 1 && p.nchunks != 1) FAIL("one chunk requested");
    check_cut(p.tiles_per_chunk, p.nchunks, Nd, columns, B, n_iso, planes, req);
    // candidate cap: c = d * n_iso + k of the last real block in 32 bits, below the "none" value
    if (p.max_candidate != Nd * n_iso - 1 || p.max_candidate > 0xFFFFFFFEll) FAIL("candidate cap");
    if ((uint32_t)p.max_candidate == 0xFFFFFFFFu) FAIL("candidate equals none");

    // the grey plan of the same launch: the same cut properties, and the 22-bit cap on a chunk's length whatever was asked for
    const int cap = fic_lsq_q_max_tiles_per_chunk(B, n_iso);
    const LsqQChunks k = lsq_q_chunk_plan(ndtiles, (columns + 31) / 32, grey_ctw(B), planes, req, FIC_LSQ_Q_NO_CAP, cap);
    grey_plans++;
    who = "grey";
    check_cut(k.tiles_per_chunk, k.nchunks, Nd, columns, B, n_iso, planes, req);
    if (k.tiles_per_chunk > cap) FAIL("chunk longer than the cap");
    if (B != 16 && (long long)k.tiles_per_chunk * 32 * n_iso > (1ll << 22)) FAIL("candidates past 22 bits");
    if (req > 0 && k.nchunks > req && k.tiles_per_chunk != cap) FAIL("more chunks than requested without the cap");
    who = "rgb";
}
#undef FAIL

// pool blocks of a w x w image: ((w / 2 - B) / (B / 4) + 1)^2
static long long pool_of(long long w, int B)
{
    const long long dw = (w / 2 - B) / (B / 4) + 1;
    return dw * dw;
}

// rows "B n_iso planes requested N_d column_tiles grey_tiles_per_chunk grey_nchunks rgb_tiles_per_chunk rgb_nchunks", recorded from
// the two rules before they became one
static long long compare_with(const char* path)
{
    FILE* f = fopen(path, "r");
    if (!f) {
        printf("FAIL cannot open %s\n", path);
        failures++;
        return 0;
    }
    char line[256];
    long long rows = 0, capped = 0;
    while (fgets(line, sizeof line, f)) {
        int B, n_iso, planes, gt, gn, rt, rn;
        long long req, Nd, ct;
        if (line[0] == '#') continue;
        if (sscanf(line, "%d %d %d %lld %lld %lld %d %d %d %d", &B, &n_iso, &planes, &req, &Nd, &ct, &gt, &gn, &rt, &rn) != 10) {
            fail("fixture row unreadable", 0, 0, 0, 0, 0, rows);
            continue;
        }
        rows++;
        const int cap = fic_lsq_q_max_tiles_per_chunk(B, n_iso);
        const LsqQChunks k = lsq_q_chunk_plan((Nd + 31) / 32, ct, grey_ctw(B), planes, req, FIC_LSQ_Q_NO_CAP, cap);
        if (k.tiles_per_chunk != gt || k.nchunks != gn) fail("grey plan differs from the recorded one", Nd, ct * 32, B, n_iso, planes, req);
        const LsqRgbQPlan p = lsq_rgb_q_plan(Nd, ct * 32, B, n_iso, planes, req);
        if (!p.ok || p.tiles_per_chunk != rt || p.nchunks != rn) fail("rgb plan differs from the recorded one", Nd, ct * 32, B, n_iso, planes, req);
        if (req > 0 && gn > req) capped++;
    }
    fclose(f);
    if (rows != 792) fail("fixture: 792 rows expected", 0, 0, 0, 0, 0, rows);
    if (capped < 4) fail("fixture has no row where the grey cap bites", 0, 0, 0, 0, 0, capped);
    return rows;
}

int main(int argc, char** argv)
{
    const int Bs[3] = {4, 8, 16}, isos[2] = {1, 8};
    const long long reqs[] = {0, 1, 2, 3, 5, 7, 8, 27, 31, 32, 33, 64, 100, 1000, 4096, 65535, 65536, 65537, 1000000, 0x7FFFFFFF};
    long long refused = 0;
    for (int bi = 0; bi < 3; bi++)
        for (int ii = 0; ii < 2; ii++) {
            const int B = Bs[bi], n_iso = isos[ii];
            // every small pool, then strides, then the pools of the timed and the largest images, and one past the grey cap
            long long nds[4200];
            int nn = 0;
            for (long long Nd = 1; Nd <= 2100; Nd++) nds[nn++] = Nd;
            for (long long Nd = 2101; Nd < 300000 && nn < 4000; Nd = Nd * 21 / 20 + 13) nds[nn++] = Nd;
            for (long long w = 256; w <= 4096; w *= 2) nds[nn++] = pool_of(w, B);
            nds[nn++] = pool_of(160, B);
            nds[nn++] = pool_of(144, B);
            nds[nn++] = (1ll << 22) + 5;
            for (int i = 0; i < nn; i++)
                for (unsigned r = 0; r < sizeof(reqs) / sizeof(reqs[0]); r++) {
                    const long long Nd = nds[i];
                    check(Nd, 1, B, n_iso, 1, reqs[r]);
                    check(Nd, (long long)(Nd % 977 + 1) * n_iso, B, n_iso, 1 + (int)(Nd % 3), reqs[r]);
                    check(Nd, 65536ll * n_iso, B, n_iso, 1, reqs[r]);
                }
            // past the cap: refused, and the edge itself accepted
            const long long edge = 0xFFFFFFFEll / n_iso;
            if (edge <= 0x7FFFFFFFll - 31) {
                check(edge, 4096, B, n_iso, 1, 0);
                if (lsq_rgb_q_plan(edge + 1, 4096, B, n_iso, 1, 0).ok) fail("cap not enforced", edge + 1, 4096, B, n_iso, 1, 0);
                else refused++;
            } else {
                if (lsq_rgb_q_plan(0x7FFFFFFFll - 30, 4096, B, n_iso, 1, 0).ok) fail("tile count not capped", 0x7FFFFFFFll - 30, 4096, B, n_iso, 1, 0);
                else refused++;
            }
            if (lsq_rgb_q_plan(0, 32, B, n_iso, 1, 0).ok || lsq_rgb_q_plan(100, 0, B, n_iso, 1, 0).ok || lsq_rgb_q_plan(100, 32, B, n_iso, 0, 0).ok)
                fail("empty geometry accepted", 0, 0, B, n_iso, 1, 0);
        }
    if (lsq_rgb_q_plan(100, 32, 32, 1, 1, 0).ok || lsq_rgb_q_plan(100, 32, 8, 4, 1, 0).ok) fail("bad B / n_iso accepted", 100, 32, 32, 4, 1, 0);
    const long long rows = argc > 1 ? compare_with(argv[1]) : 0;
    if (argc <= 1) fail("no fixture given", 0, 0, 0, 0, 0, 0);
    printf("%lld plans checked, %lld grey plans, %lld refusals at the cap, %lld recorded rows compared\n%lld failures\n", plans, grey_plans, refused, rows, failures);
    return failures ? 1 : 0;
}
