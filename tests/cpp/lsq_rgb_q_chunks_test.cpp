// lsq_rgb_q_chunks_test.cpp -- stand-alone host check of the pool-chunk arithmetic of the matrix-core joint-RGB least-squares
// sweep (csrc/fic_lsq_rgb_q_chunks.h): over (N_d, requested chunks, B, n_iso, columns, planes) from
// N_d = 1 up to the pools of 4096 x 4096 images it checks that no chunk is empty, that the chunks cover every domain tile exactly
// once and in order, that the slot count is the chunk count, that the count never exceeds what was asked for (nor the launcher's
// limit), that the largest candidate a chunk can write fits the 32 bits of the per-lane minima beside their "none" value, and
// that pools past that cap are refused.  Built by tests/test_rgb_lsq_q_bound.py with the host compiler and its sanitizers; never
// runs on a GPU.
#include <stdint.h>
#include <stdio.h>

#include "../../fractal-image-compression_amd/csrc/fic_lsq_rgb_q_chunks.h"

static long long failures = 0, plans = 0;

static void fail(const char* what, long long Nd, long long columns, int B, int n_iso, int planes, long long req)
{
    if (failures < 20) printf("FAIL %s: Nd=%lld columns=%lld B=%d n_iso=%d planes=%d requested=%lld\n", what, Nd, columns, B, n_iso, planes, req);
    failures++;
}

static void check(long long Nd, long long columns, int B, int n_iso, int planes, long long req)
{
    const LsqRgbQPlan p = lsq_rgb_q_plan(Nd, columns, B, n_iso, planes, req);
    plans++;
    if (!p.ok) return fail("refused", Nd, columns, B, n_iso, planes, req);
    const long long ndtiles = (Nd + 31) / 32;
    if (p.ndtiles != ndtiles) fail("ndtiles", Nd, columns, B, n_iso, planes, req);
    if (p.nchunks < 1 || p.tiles_per_chunk < 1) return fail("counts", Nd, columns, B, n_iso, planes, req);
    if (p.nslots != p.nchunks) fail("slots", Nd, columns, B, n_iso, planes, req);
    if (p.nchunks > FIC_LSQ_RGB_Q_MAX_CHUNKS || p.nchunks > ndtiles) fail("too many chunks", Nd, columns, B, n_iso, planes, req);
    if (req > 0 && p.nchunks > req) fail("more chunks than requested", Nd, columns, B, n_iso, planes, req);
    if (req == 1 && p.nchunks != 1) fail("one chunk requested", Nd, columns, B, n_iso, planes, req);
    // the launcher's conditions
    if ((long long)p.tiles_per_chunk * (p.nchunks - 1) >= ndtiles || (long long)p.tiles_per_chunk * p.nchunks < ndtiles)
        fail("launcher", Nd, columns, B, n_iso, planes, req);
    // coverage, in order, nothing empty: walk the chunks as the kernel does (all of a small plan; both ends of a large one, whose
    // middle follows from the launcher's conditions above: chunk c starts at c * tiles_per_chunk and is full)
    for (int part = 0; part < 2; part++) {
        const int c0 = part == 0 ? 0 : (p.nchunks > 4096 ? p.nchunks - 2048 : p.nchunks);
        const int c1 = part == 0 ? (p.nchunks > 4096 ? 2048 : p.nchunks) : p.nchunks;
        long long next = (long long)c0 * p.tiles_per_chunk;
        for (int c = c0; c < c1; c++) {
            int t0, t1;
            lsq_rgb_q_chunk_tiles(p, c, &t0, &t1);
            if (t1 <= t0) fail("empty chunk", Nd, columns, B, n_iso, planes, req);
            if (t0 != next) fail("gap or overlap", Nd, columns, B, n_iso, planes, req);
            if (t1 > ndtiles) fail("past the pool", Nd, columns, B, n_iso, planes, req);
            if ((long long)t0 * 32 >= Nd) fail("chunk without a real row", Nd, columns, B, n_iso, planes, req);   // its slot is written
            next = t1;
            if (c == p.nchunks - 1 && t1 != ndtiles) fail("tail not covered", Nd, columns, B, n_iso, planes, req);
        }
    }
    // candidate cap: c = d * n_iso + k of the last real block in 32 bits, below the "none" value
    if (p.max_candidate != Nd * n_iso - 1 || p.max_candidate > 0xFFFFFFFEll) fail("candidate cap", Nd, columns, B, n_iso, planes, req);
    if ((uint32_t)p.max_candidate == 0xFFFFFFFFu) fail("candidate equals none", Nd, columns, B, n_iso, planes, req);
}

// pool blocks of a w x w image: ((w / 2 - B) / (B / 4) + 1)^2
static long long pool_of(long long w, int B)
{
    const long long dw = (w / 2 - B) / (B / 4) + 1;
    return dw * dw;
}

int main()
{
    const int Bs[3] = {4, 8, 16}, isos[2] = {1, 8};
    const long long reqs[] = {0, 1, 2, 3, 5, 7, 8, 27, 31, 32, 33, 64, 100, 1000, 4096, 65535, 65536, 65537, 1000000, 0x7FFFFFFF};
    long long refused = 0;
    for (int bi = 0; bi < 3; bi++)
        for (int ii = 0; ii < 2; ii++) {
            const int B = Bs[bi], n_iso = isos[ii];
            // every small pool, then strides, then the pools of the timed and the largest images
            long long nds[4200];
            int nn = 0;
            for (long long Nd = 1; Nd <= 2100; Nd++) nds[nn++] = Nd;
            for (long long Nd = 2101; Nd < 300000 && nn < 4000; Nd = Nd * 21 / 20 + 13) nds[nn++] = Nd;
            for (long long w = 256; w <= 4096; w *= 2) nds[nn++] = pool_of(w, B);
            nds[nn++] = pool_of(160, B);
            nds[nn++] = pool_of(144, B);
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
    printf("%lld plans checked, %lld refusals at the cap\n%lld failures\n", plans, refused, failures);
    return failures ? 1 : 0;
}
