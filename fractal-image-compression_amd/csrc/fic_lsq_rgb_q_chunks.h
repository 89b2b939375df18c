// fic_lsq_rgb_q_chunks.h -- pool chunks of the matrix-core joint-RGB least-squares sweep (k_sweep_lsq_rgb_q, fic_lsq_rgb_q.hip,
// DESIGN.md section 4.22).  Plain C++ without HIP: shared by the launcher, by fic_capi_rgb_lsq.cpp and by the host check
// tests/cpp/lsq_rgb_q_chunks_test.cpp, which runs it under the address and undefined-behaviour sanitizers.
//
// The pool is cut in domain tiles of 32 blocks.  A chunk is tiles_per_chunk consecutive tiles (the last chunk may be shorter,
// never empty), so every (chunk, range block) slot is written and k_finalize_lsq_rgb reads nslots = nchunks slots per range
// block.  The sweep keeps its minima as per-lane (E, c) pairs with c the GLOBAL candidate pool block * n_iso + isometry in 32
// unsigned bits (0xFFFFFFFF stands for "none"), so the only cap is on the pool as a whole: N_d * n_iso <= 2^32 - 2.  No cap on
// the length of a chunk follows from it (unlike the grey sweep's 22-bit field), and the codebook cannot depend on the cut.
#pragma once
#include <stdint.h>

#define FIC_LSQ_RGB_Q_WPG 4                    // waves per workgroup of k_sweep_lsq_rgb_q (independent: no barrier)
#define FIC_LSQ_RGB_Q_MAX_CHUNKS 65536         // slots per range block the launcher accepts

struct LsqRgbQPlan {
    int ok;                                    // 0: the geometry is refused (B, n_iso, an empty pool or the candidate cap)
    int ndtiles, tiles_per_chunk, nchunks, nslots;
    long long max_candidate;                   // the largest c the sweep can write: N_d * n_iso - 1
};

// column tiles (x32 columns) one wave keeps in registers, by NK = 3 n / 16 K-steps: 4 / 2 / 1 at B = 4 / 8 / 16
inline int lsq_rgb_q_ctw(int B) { return B == 4 ? 4 : (B == 8 ? 2 : 1); }

// `columns` = range blocks * n_iso of the launch, `requested` = option "chunks" (<= 0: automatic).  Automatic count, the fill /
// balance rule of the grey sweep (a chunk's first tile is evaluated in full, 1024 exact pairs per column tile of every wave):
//  fill:    fewer waves than the chip holds at two per SIMD (2048): split until they exist, down to chunks of 8 domain tiles;
//  balance: up to four such rounds of waves (8192), but only with chunks of 500 domain tiles or more.
inline LsqRgbQPlan lsq_rgb_q_plan(long long Nd, long long columns, int B, int n_iso, int planes, long long requested)
{
    LsqRgbQPlan p = {0, 0, 0, 0, 0, -1};
    if ((B != 4 && B != 8 && B != 16) || (n_iso != 1 && n_iso != 8) || Nd < 1 || columns < 1 || planes < 1) return p;
    if (Nd > (0xFFFFFFFEll / n_iso) || Nd > 0x7FFFFFFFll - 31) return p;          // c in 32 bits beside the "none" value; tiles in int
    const long long ndtiles = (Nd + 31) / 32;
    long long nc = requested;
    if (nc <= 0) {
        const long long ctw = lsq_rgb_q_ctw(B);
        const long long ct = (columns + 31) / 32;
        const long long base_waves = (ct + ctw - 1) / ctw * planes;               // wave tasks per chunk
        long long fill = (2048 + base_waves - 1) / base_waves, bal = (8192 + base_waves - 1) / base_waves;
        if (fill > ndtiles / 8) fill = ndtiles / 8;
        if (bal > ndtiles / 500) bal = ndtiles / 500;
        nc = fill > bal ? fill : bal;
    }
    if (nc > ndtiles) nc = ndtiles;
    if (nc > FIC_LSQ_RGB_Q_MAX_CHUNKS) nc = FIC_LSQ_RGB_Q_MAX_CHUNKS;
    if (nc < 1) nc = 1;
    const long long tpc = (ndtiles + nc - 1) / nc;
    p.ndtiles = (int)ndtiles;
    p.tiles_per_chunk = (int)tpc;
    p.nchunks = (int)((ndtiles + tpc - 1) / tpc);                                  // no empty chunk: every slot gets written
    p.nslots = p.nchunks;
    p.max_candidate = Nd * n_iso - 1;
    p.ok = 1;
    return p;
}

// domain tiles [*t0, *t1) of chunk `chunk` of a plan: what the kernel computes
inline void lsq_rgb_q_chunk_tiles(const LsqRgbQPlan& p, int chunk, int* t0, int* t1)
{
    const long long a = (long long)chunk * p.tiles_per_chunk;
    long long b = a + p.tiles_per_chunk;
    if (b > p.ndtiles) b = p.ndtiles;
    *t0 = (int)a;
    *t1 = (int)b;
}
