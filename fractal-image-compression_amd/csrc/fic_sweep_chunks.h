// fic_sweep_chunks.h -- pool chunks of every sweep but the two matrix-core least-squares ones (those: fic_lsq_q_chunks.h).
// Plain C++ without HIP, integers in and out: the callers (fic_capi.cpp, fic_capi_rgb.cpp, fic_capi_rgb_lsq.cpp) work out the
// wave tasks or workgroups per chunk from their geometry, tests/cpp/sweep_chunks_test.cpp runs the rules under the address and
// undefined-behaviour sanitizers and against tests/golden/sweep_chunks.txt.  `requested` is the option "chunks" (<= 0:
// automatic).  Every rule ends the same way: the count is clamped to the pool, the length follows from the count (rounded up
// to what the kernel consumes at once) and the count from the length, so no chunk is empty and the chunks cover the pool.
#pragma once

struct SweepChunks {
    int len, nchunks;                // pool blocks (VALU sweeps) or domain tiles of 32 blocks (matrix-core sweeps) per chunk
};

inline long long sweep_ceil_div(long long a, long long b) { return (a + b - 1) / b; }
inline SweepChunks sweep_chunks_cut(long long pool, long long nc, long long step)
{
    if (nc > pool) nc = pool;
    if (nc < 1) nc = 1;
    const long long len = sweep_ceil_div(sweep_ceil_div(pool, nc), step) * step;
    return SweepChunks{(int)len, (int)sweep_ceil_div(pool, len)};
}

// The VALU sweeps k_sweep_fast, k_sweep_d4 and k_sweep_lsq_fast over a pool of Nd blocks; `base_waves` = wave tasks per chunk.
// Measured (profiles/r01l_chunk_sweep.txt): every chunk pays a start-up (its first block is evaluated exactly and tau
// restarts), so chunks stay >= 4096 blocks while aiming at `target` = 49152 (~48 K) wave tasks for load balance; only a launch
// that could not otherwise fill the chip (one small image) splits finer.  k_sweep_lsq_fast pays more per start-up -- its
// epilogue is 64-bit integer work -- and asks for `target` = 6144 wave tasks, about one resident round
// (profiles/lsq_timing.txt).  `even`: the sweep consumes blocks in pairs (all but k_sweep_d4).
#define FIC_VALU_CHUNK_TARGET 49152
#define FIC_LSQ_FAST_CHUNK_TARGET 6144
inline SweepChunks valu_chunks(long long Nd, long long base_waves, long long requested, long long target, bool even)
{
    long long nc = requested;
    if (nc <= 0) {
        const long long want = sweep_ceil_div(target, base_waves);
        long long cap = Nd / 4096;
        if (cap < 1) cap = 1;
        nc = want < cap ? want : cap;
        if (base_waves * nc < 4096) {
            long long cap2 = Nd / 512;
            if (cap2 < 1) cap2 = 1;
            const long long fill = sweep_ceil_div(4096, base_waves);
            nc = fill < cap2 ? fill : cap2;
        }
    }
    return sweep_chunks_cut(Nd, nc, even ? 2 : 1);
}

// The cross-check matrix-core sweeps ("sweep" = 3 / 4) over ndtiles domain tiles; `base_wg` = workgroups per chunk.
inline SweepChunks xcheck_chunks(long long ndtiles, long long base_wg, long long requested)
{
    long long nc = requested;
    if (nc <= 0) {
        const long long want = sweep_ceil_div(4096, base_wg);                  // ~4 resident per CU x 256 CUs x 4
        long long cap = ndtiles / 256;                                         // >= 256 domain tiles per chunk: start-up < 10 %
        if (cap < 1) cap = 1;
        nc = want < cap ? want : cap;
        if (base_wg * nc < 1024) {                                             // one small image: fill the chip first,
            long long cap2 = ndtiles / 32;                                     // even at a higher per-chunk start-up share
            if (cap2 < 1) cap2 = 1;
            const long long fill = sweep_ceil_div(1024, base_wg);
            nc = fill < cap2 ? fill : cap2;
        }
    }
    return sweep_chunks_cut(ndtiles, nc, 1);
}

// k_sweep_q, grey ("sweep" = 6, the default full search) and joint RGB ("sweep" = 2), over ndtiles domain tiles; `base_wg` =
// workgroups per chunk, `resident` = workgroups the chip holds at once, `unroll` = tiles per iteration of the sweep loop.
// Two reasons to split the pool into chunks, each with its own price (a chunk starts with theta unset: until its first good
// candidate has been evaluated every pair of every tile is queued -- tens of tiles' worth of work):
//  fill:    fewer workgroups than the chip holds at once: split until two rounds of them exist, but keep >= `min_tiles` tiles
//           per chunk;
//  balance: the kernel ends with its slowest wave, and one round of equally long waves leaves ~25 % of the wave-cycles idle
//           (profiles/r02w_chunk_count_sweep.txt): aim for 8 rounds, but only with chunks long enough (>= 1024 tiles) that the
//           start-up is noise.
// min_tiles (one image, profiles/r03n_single_image_chunk_count_sweep.json): a chunk restarts theta, and what that costs against
// the parallelism it buys depends on the columns per range block -- grey with 8 isometries: 30, chunks below ~30 domain tiles
// lose (512x512: 0.086 ms per encode at 16 chunks, 0.092-0.094 at 28); grey with 1 isometry: 14, 14-tile chunks still gain
// (0.060 at 35 chunks, 0.061 at 28, 0.076 at 16); joint RGB: 16.
inline int q_min_tiles_grey(int n_iso) { return n_iso == 8 ? 30 : 14; }
#define FIC_RGB_Q_MIN_TILES 16
inline SweepChunks q_chunks(long long ndtiles, long long base_wg, long long resident, long long min_tiles, long long unroll,
                            long long requested)
{
    long long nc = requested;
    if (nc <= 0) {
        long long fill = base_wg < resident ? sweep_ceil_div(2 * resident, base_wg) : 1;
        if (fill > ndtiles / min_tiles) fill = ndtiles / min_tiles;
        long long bal = sweep_ceil_div(8 * resident, base_wg);
        if (bal > ndtiles / 1024) bal = ndtiles / 1024;
        nc = fill > bal ? fill : bal;
    }
    return sweep_chunks_cut(ndtiles, nc, unroll);      // whole iterations of the unrolled sweep loop
}

// k_sweep_lsq_rgb_fast over a pool of Nd blocks; `tasks` = wave tasks per chunk.  About one resident round of waves (6144 wave
// tasks, profiles/lsq_timing.txt), chunks of 16 pool blocks or more, never more than 4096 chunks; "chunks" overrides the first two.
inline SweepChunks rgb_lsq_fast_chunks(long long Nd, long long tasks, long long requested)
{
    long long nc = requested > 0 ? requested : sweep_ceil_div(6144, tasks);
    const long long cap = requested > 0 ? Nd : (Nd / 16 > 1 ? Nd / 16 : 1);
    if (nc > cap) nc = cap;
    if (nc > 4096) nc = 4096;
    return sweep_chunks_cut(Nd, nc, 1);
}
