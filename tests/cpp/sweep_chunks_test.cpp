// sweep_chunks_test.cpp -- stand-alone host check of csrc/fic_sweep_chunks.h, the pool-chunk rules of the VALU sweeps, the
// cross-check matrix-core sweeps, k_sweep_q (grey and joint RGB) and k_sweep_lsq_rgb_fast.  Given tests/golden/sweep_chunks.txt
// it compares every rule with the recorded row (what the C ABI computed before the rules had a header of their own); then, over
// every pool size from 1 to 2100 and strides beyond, it checks what the launchers and kernels rely on: no empty chunk, the chunks
// cover the pool once and in order, even lengths / whole unrolled iterations where asked, never more chunks than pool entries or
// than requested, one chunk when one is requested, at most 4096 chunks of k_sweep_lsq_rgb_fast, and the predicate
// fic_launch_sweep_lsq_fast applies to its arguments.  Built by tests/test_sweep_chunks.py with the host compiler and its
// sanitizers; never runs on a GPU.
#include <stdio.h>

#include "../../fractal-image-compression_amd/csrc/fic_sweep_chunks.h"

static long long failures = 0, cuts = 0;

static void fail(const char* rule, const char* what, long long pool, long long base, long long req)
{
    if (failures < 20) printf("FAIL %s %s: pool=%lld base=%lld requested=%lld\n", rule, what, pool, base, req);
    failures++;
}

// what every rule owes its kernel; `step`: the length is a multiple of it
#define FAIL(what) fail(rule, what, pool, base, req)
static void check_cut(const char* rule, SweepChunks k, long long pool, long long base, long long req, long long step)
{
    cuts++;
    const long long len = k.len, nc = k.nchunks;
    if (len < 1 || nc < 1) return FAIL("counts");
    if (len % step) FAIL("length no multiple of the step");
    if (nc > pool) FAIL("more chunks than pool entries");
    if (req > 0 && nc > req) FAIL("more chunks than requested");
    if (req == 1 && nc != 1) FAIL("one chunk requested");
    if (!(len * (nc - 1) < pool && pool <= len * nc)) FAIL("empty chunk or pool not covered");
    // walk the chunks as the kernels do: chunk c is [c * len, min(pool, (c + 1) * len)) (all of a small cut; both ends of a
    // large one, whose middle chunks are full by the line above)
    long long next = 0;
    for (long long c = 0; c < nc; c++) {
        if (c == 16 && nc > 32) {
            c = nc - 16;
            next = c * len;
        }
        const long long a = c * len, b = a + len < pool ? a + len : pool;
        if (b <= a) FAIL("empty chunk");
        if (a != next) FAIL("gap or overlap");
        next = b;
    }
    if (next != pool) FAIL("tail not covered");
}
#undef FAIL

static void properties()
{
    const long long reqs[] = {0, 1, 2, 3, 5, 7, 8, 27, 31, 32, 33, 64, 100, 1000, 4096, 65535, 65536, 65537, 1000000, 0x7FFFFFFF};
    const long long bases[] = {1, 7, 512, 513, 4096, 6144, 100000};
    long long pools[4200];
    int np = 0;
    for (long long p = 1; p <= 2100; p++) pools[np++] = p;
    for (long long p = 2101; p < 20000000 && np < 4200; p = p * 21 / 20 + 13) pools[np++] = p;
    for (int i = 0; i < np; i++)
        for (long long req : reqs)
            for (long long base : bases) {
                const long long pool = pools[i];
                for (int even = 0; even < 2; even++)
                    for (int t = 0; t < 2; t++) {
                        const long long target = t ? FIC_LSQ_FAST_CHUNK_TARGET : FIC_VALU_CHUNK_TARGET;
                        const SweepChunks k = valu_chunks(pool, base, req, target, even != 0);
                        check_cut(even ? "valu_chunks even" : "valu_chunks", k, pool, base, req, even ? 2 : 1);
                        // fic_launch_sweep_lsq_fast's own words
                        if (even && !(k.len >= 2 && k.len % 2 == 0 && (long long)k.len * (k.nchunks - 1) < pool && pool <= (long long)k.len * k.nchunks))
                            fail("valu_chunks", "the least-squares launcher's predicate", pool, base, req);
                    }
                check_cut("xcheck_chunks", xcheck_chunks(pool, base, req), pool, base, req, 1);
                const long long qs[5][3] = {{256, 14, 2}, {512, 30, 2}, {768, 16, 2}, {512, 14, 1}, {512, 16, 4}};   // resident, min_tiles, unroll
                for (const auto& q : qs) check_cut("q_chunks", q_chunks(pool, base, q[0], q[1], q[2], req), pool, base, req, q[2]);
                const SweepChunks r = rgb_lsq_fast_chunks(pool, base, req);
                check_cut("rgb_lsq_fast_chunks", r, pool, base, req, 1);
                if (r.nchunks > 4096) fail("rgb_lsq_fast_chunks", "more than 4096 chunks", pool, base, req);
            }
}

// the rows of tests/golden/sweep_chunks.txt (its header names the columns)
static long long compare_with(const char* path)
{
    FILE* f = fopen(path, "r");
    if (!f) {
        printf("FAIL cannot open %s\n", path);
        failures++;
        return 0;
    }
    char line[512];
    long long rows = 0;
    while (fgets(line, sizeof line, f)) {
        if (line[0] == '#') continue;
        int B, n_iso, w, planes, span, want[14];
        long long req, Nd, ndtiles, valu_waves, d4_waves, xcheck_wg, q_wg, resident, rgb_q_wg, tasks;
        if (sscanf(line, "%d %d %d %d %d %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %d %d %d %d %d %d %d %d %d %d %d %d %d %d", &B, &n_iso, &w,
                   &planes, &span, &req, &Nd, &ndtiles, &valu_waves, &d4_waves, &xcheck_wg, &q_wg, &resident, &rgb_q_wg, &tasks, &want[0], &want[1],
                   &want[2], &want[3], &want[4], &want[5], &want[6], &want[7], &want[8], &want[9], &want[10], &want[11], &want[12], &want[13]) != 29) {
            fail("table", "row unreadable", 0, 0, rows);
            continue;
        }
        rows++;
        const int unroll = 2;                      // fic_q_unroll: two fragment buffers swap roles
        const SweepChunks got[7] = {valu_chunks(Nd, valu_waves, req, FIC_VALU_CHUNK_TARGET, true),
                                    valu_chunks(Nd, d4_waves, req, FIC_VALU_CHUNK_TARGET, false),
                                    valu_chunks(Nd, valu_waves, req, FIC_LSQ_FAST_CHUNK_TARGET, true),
                                    xcheck_chunks(ndtiles, xcheck_wg, req),
                                    q_chunks(ndtiles, q_wg, resident, q_min_tiles_grey(n_iso), unroll, req),
                                    q_chunks(ndtiles, rgb_q_wg, resident, FIC_RGB_Q_MIN_TILES, unroll, req),
                                    rgb_lsq_fast_chunks(Nd, tasks, req)};
        static const char* const names[7] = {"valu", "d4", "lsq_fast", "xcheck", "q", "rgb_q", "rgb_lsq_fast"};
        for (int i = 0; i < 7; i++)
            if (got[i].len != want[2 * i] || got[i].nchunks != want[2 * i + 1]) {
                if (failures < 20)
                    printf("FAIL %s differs from the recorded row %lld (B=%d n_iso=%d w=%d planes=%d span=%d requested=%lld): {%d, %d}, recorded {%d, %d}\n",
                           names[i], rows, B, n_iso, w, planes, span, req, got[i].len, got[i].nchunks, want[2 * i], want[2 * i + 1]);
                failures++;
            }
    }
    fclose(f);
    if (rows != 1620) fail("table", "1620 rows expected", 0, 0, rows);
    return rows;
}

int main(int argc, char** argv)
{
    const long long rows = argc > 1 ? compare_with(argv[1]) : 0;
    if (argc <= 1) fail("table", "no fixture given", 0, 0, 0);
    properties();
    printf("%lld recorded rows compared, %lld cuts checked\n%lld failures\n", rows, cuts, failures);
    return failures ? 1 : 0;
}
