// fic_lsq_q_chunks.h -- pool chunks of the two matrix-core least-squares sweeps: k_sweep_lsq_q (grey, fic_lsq_q.hip, DESIGN.md
// section 4.21) and k_sweep_lsq_rgb_q (joint RGB, fic_lsq_rgb_q.hip, section 4.22).  Plain C++ without HIP: shared by the two
// launchers, by fic_capi.cpp and fic_capi_rgb_lsq.cpp and by the host check tests/cpp/lsq_q_chunks_test.cpp, which runs it under
// the address and undefined-behaviour sanitizers.
//
// The pool is cut in domain tiles of 32 blocks.  A chunk is tiles_per_chunk consecutive tiles (the last chunk may be shorter,
// never empty), so every (chunk, range block) slot is written and the finalise kernel reads nchunks slots per range block.
//  grey: B = 4 / 8 number a chunk's candidates in 22 bits beside E in a 64-bit minimum, which caps the LENGTH of a chunk; a pool
//        longer than requested * cap gets more chunks than were asked for.
//  RGB:  per-lane (E, c) pairs, c the GLOBAL candidate in 32 unsigned bits (0xFFFFFFFF: "none"): the only cap is on the pool,
//        N_d * n_iso <= 2^32 - 2, none on a chunk's length; the launcher takes at most FIC_LSQ_RGB_Q_MAX_CHUNKS slots.
// The codebook cannot depend on the cut in either.
#pragma once
#include <stdint.h>

#define FIC_LSQ_RGB_Q_WPG 4                    // waves per workgroup of k_sweep_lsq_rgb_q (independent: no barrier)
#define FIC_LSQ_RGB_Q_MAX_CHUNKS 65536         // slots per range block the launcher accepts
#define FIC_LSQ_Q_NO_CAP 0x7FFFFFFFll          // "no cap" on the chunk count or on a chunk's length (both are ints)

struct LsqQChunks {
    int tiles_per_chunk, nchunks;
};

// The one chunk plan.  `ct` = column tiles (x32 columns) of the launch, `ctw` = column tiles one wave keeps, `requested` =
// option "chunks" (<= 0: automatic).  A chunk's start costs a full first tile (1024 exact pairs per column tile of every wave),
// so the automatic count has two reasons to split, each with its own floor under the chunk length (measured,
// profiles/lsq_q_timing.txt part 2, DESIGN.md 4.21 "Chunk policy"):
//  fill:    fewer waves than the chip holds at two per SIMD (2048): split until they exist, down to chunks of 8 domain tiles;
//  balance: up to four such rounds of waves (8192), but only with chunks of 500 domain tiles or more.
// Then the count is clamped to [1, min(ndtiles, max_chunks)], the length to max_tiles_per_chunk; the count follows from it.
inline LsqQChunks lsq_q_chunk_plan(long long ndtiles, long long ct, long long ctw, int planes, long long requested,
                                   long long max_chunks, long long max_tiles_per_chunk)
{
    long long nc = requested;
    if (nc <= 0) {
        const long long base_waves = (ct + ctw - 1) / ctw * planes;               // wave tasks per chunk
        long long fill = (2048 + base_waves - 1) / base_waves, bal = (8192 + base_waves - 1) / base_waves;
        if (fill > ndtiles / 8) fill = ndtiles / 8;
        if (bal > ndtiles / 500) bal = ndtiles / 500;
        nc = fill > bal ? fill : bal;
    }
    if (nc > ndtiles) nc = ndtiles;
    if (nc > max_chunks) nc = max_chunks;
    if (nc < 1) nc = 1;
    long long tpc = (ndtiles + nc - 1) / nc;
    if (tpc > max_tiles_per_chunk) tpc = max_tiles_per_chunk;
    return LsqQChunks{(int)tpc, (int)((ndtiles + tpc - 1) / tpc)};                // no empty chunk: every slot gets written
}

// what both launchers ask of a cut: no empty chunk, and the chunks cover the pool
inline bool lsq_q_chunks_cover(long long ndtiles, long long tiles_per_chunk, long long nchunks)
{
    return tiles_per_chunk >= 1 && nchunks >= 1 && tiles_per_chunk * (nchunks - 1) < ndtiles && tiles_per_chunk * nchunks >= ndtiles;
}

// domain tiles [*t0, *t1) of chunk `chunk`: what the kernels compute
inline void lsq_q_chunk_tiles(int ndtiles, int tiles_per_chunk, int chunk, int* t0, int* t1)
{
    const long long a = (long long)chunk * tiles_per_chunk;
    long long b = a + tiles_per_chunk;
    if (b > ndtiles) b = ndtiles;
    *t0 = (int)a;
    *t1 = (int)b;
}

// grey, B = 4 / 8: a chunk's candidates are numbered in 22 bits beside E in the 64-bit minimum
inline int fic_lsq_q_max_tiles_per_chunk(int B, int n_iso) { return B == 16 ? (1 << 26) : (1 << 17) / n_iso; }

// ---- joint RGB: geometry and candidate-cap refusal around the plan ------------------------------------------------------------
struct LsqRgbQPlan {
    int ok;                                    // 0: the geometry is refused (B, n_iso, an empty pool or the candidate cap)
    int ndtiles, tiles_per_chunk, nchunks, nslots;
    long long max_candidate;                   // the largest c the sweep can write: N_d * n_iso - 1
};

// column tiles (x32 columns) one wave keeps in registers, by NK = 3 n / 16 K-steps: 4 / 2 / 1 at B = 4 / 8 / 16
inline int lsq_rgb_q_ctw(int B) { return B == 4 ? 4 : (B == 8 ? 2 : 1); }

// `columns` = range blocks * n_iso of the launch
inline LsqRgbQPlan lsq_rgb_q_plan(long long Nd, long long columns, int B, int n_iso, int planes, long long requested)
{
    LsqRgbQPlan p = {0, 0, 0, 0, 0, -1};
    if ((B != 4 && B != 8 && B != 16) || (n_iso != 1 && n_iso != 8) || Nd < 1 || columns < 1 || planes < 1) return p;
    if (Nd > (0xFFFFFFFEll / n_iso) || Nd > 0x7FFFFFFFll - 31) return p;          // c in 32 bits beside the "none" value; tiles in int
    const long long ndtiles = (Nd + 31) / 32;
    const LsqQChunks k = lsq_q_chunk_plan(ndtiles, (columns + 31) / 32, lsq_rgb_q_ctw(B), planes, requested, FIC_LSQ_RGB_Q_MAX_CHUNKS, FIC_LSQ_Q_NO_CAP);
    p.ndtiles = (int)ndtiles;
    p.tiles_per_chunk = k.tiles_per_chunk;
    p.nchunks = k.nchunks;
    p.nslots = p.nchunks;
    p.max_candidate = Nd * n_iso - 1;
    p.ok = 1;
    return p;
}
