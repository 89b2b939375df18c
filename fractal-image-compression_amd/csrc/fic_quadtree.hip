// fic_quadtree.hip -- quadtree (variable block size) codec on the device, grey and joint RGB: collage error per range
// block, the split decision + leaf compaction, and the decoder's paint of leaves of mixed size.  An extension like
// n_iso = 8: the reference encodes with one block size (FC:14).  gfx950 (MI355X / CDNA4) only, wave64; -ffp-contract=off
// like every other translation unit (the paint arithmetic is k_decode_paint's / k_decode_paint_rgb's, one rounding per
// operation).  DESIGN.md sections 4.13 (grey), 4.14 (colour) and 4.17 (colour with the 8 isometries).
//
// The kernels that touch pixels are templated on the pixel format (QtGrey / QtRgb / QtRgbIso, fic_launch.h) and share their
// indexing, their atomics and the reduction of the decoder's squares; only the per-pixel arithmetic of a block row is written
// per pixel type (qt_row_sse / qt_paint_row on bytes: qt_row_values; on packed ARGB: rgb_domain_seg + rgb_row_coef /
// rgb_paint_px, fic_devfn.h).  QtRgb passes the constant isometry 0 to the ARGB code, which then is the code it always was.
//
//   k_leaf_sse<Fmt, B>       SSE of the quantised row of every range block of one level against the original image (colour:
//                            summed over the three channels)
//   k_qt_count / k_qt_scan / k_qt_scatter<Fmt>
//                            top-down split of every top-level (B_max) block, leaf count, exclusive scan, ordered scatter
//   k_decode_paint_leaves<Fmt, B>
//                            one decoder paint of the leaves of one level (three launches per iteration, one per level)
//   k_qt_keys / k_qt_select_hist / k_qt_select_final / k_qt_tree_stats
//                            encode to a leaf budget: the split keys e(v), a radix select of the key that
//                            the budget falls on and its threshold, the collage SSE and the leaves per level of the tree
//   k_qt_rd_keys / k_qt_select_hist_w / k_qt_select_final_w
//                            encode by rate-distortion pruning: the keys e(v) and gains G_v of min D + lambda N,
//                            and the select of the key at which the summed gain reaches an SSE target
//   k_qt_resolve<Fmt> / k_qt_paint_planes<Fmt, S, kCollage>
//                            decode and collage of a batch from the encoder's leaf table as it stands on the device (DESIGN.md
//                            4.25): every row checked and resolved, then one paint of all levels and planes per iteration
// The walkers (k_qt_count, k_qt_scatter, k_qt_tree_stats) take the split rule as a type: QtByThreshold (4.13) or QtByKey (4.23).
// Every encoder kernel takes a batch of planes (FicQtPlanes in fic_launch.h): the plane is a grid dimension, so no
// workgroup spans two planes, and every parameter of a split rule -- threshold, rank, SSE target, lambda -- is read per plane
// from device memory.  That is the only mode: one host pipeline (qt_tree_run, fic_capi_quadtree.cpp) drives these kernels for
// its two front ends, the one-shot entries (a batch of one plane) and the batched handle (fic_capi_qt_ctx.cpp).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fic_device.h"
#include "fic_launch.h"
#include "fic_devfn.h"

// The quantised row's value at every pixel of a range block row, as k_decode_paint computes it (FC:394-402):
//   a = (float) qa / 100f, b = (float) qb, value = clamp((int) fl(fl(a * d) + b)),
// d the winner's domain pixel (isometry applied) in the 2:1-scaled image `scaled`.
// A row is evaluated in segments of S pixels from x0 on (S = B, x0 = 0 up to B = 16: the whole row).
template <int B, int S>
__device__ __forceinline__ void qt_row_values(const uint8_t* __restrict__ scaled, const FicGeom& g, int gi, int k, int ry, int x0,
                                              float a, float b, int (&value)[S])
{
    const int c = gi % g.Dw, r = gi / g.Dw;
    const uint8_t* dom = scaled + (size_t)(r * g.abstand) * g.Ws + c * g.abstand;
    uint8_t dpx[S];
    if (k == 0) {
        __builtin_memcpy(dpx, dom + (size_t)ry * g.Ws + x0, S);
    } else {
        int ax, bx_, cx, ay, by_, cy;
        iso_affine(k, B - 1, ax, bx_, cx, ay, by_, cy);
        const int sx = ay * g.Ws + ax, s0 = (cy + by_ * ry) * g.Ws + cx + bx_ * ry + sx * x0;
#pragma unroll
        for (int x = 0; x < S; x++) dpx[x] = dom[s0 + sx * x];
    }
#pragma unroll
    for (int x = 0; x < S; x++) {
        int v = java_f2i(__fadd_rn(__fmul_rn(a, (float)dpx[x]), b));
        value[x] = v < 0 ? 0 : (v > 255 ? 255 : v);
    }
}

// The sum over one pixel row `prow` of a range block of (orig - value)^2, grey: q = {qa, qb} of the block's row, k its isometry.
template <int B>
__device__ __forceinline__ uint32_t qt_row_sse(const uint8_t* __restrict__ prow, const uint8_t* __restrict__ scaled, const FicGeom& g,
                                               int gi, int k, int ry, const int32_t* __restrict__ q)
{
    int value[B];
    qt_row_values<B, B>(scaled, g, gi, k, ry, 0, __fdiv_rn((float)q[0], 100.0f), (float)q[1], value);
    uint32_t s = 0;
#pragma unroll
    for (int x = 0; x < B; x++) {
        const int d = (int)prow[x] - value[x];
        s += (uint32_t)(d * d);
    }
    return s;
}

// ---------------------------------------------------------------------------------------------
// Joint RGB.  The paint arithmetic of k_decode_paint_rgb (rgb_row_coef / rgb_paint_px, fic_devfn.h) on the
// packed ARGB pixels; d is the domain pixel in the scaleImageRGB copy (FC:901-962), origin (c * B/4, r * B/4).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t rgb_sq(int32_t cur, int vR, int vG, int vB)
{
    const int dR = ((cur >> 16) & 0xff) - vR, dG = ((cur >> 8) & 0xff) - vG, dB = (cur & 0xff) - vB;
    return (uint32_t)(dR * dR + dG * dG + dB * dB);
}
__device__ __forceinline__ const int32_t* rgb_domain_row(const int32_t* __restrict__ scaled, const FicGeom& g, int gi, int ry)
{
    const int c = gi % g.Dw, r = gi / g.Dw;
    return scaled + (size_t)(r * g.abstand + ry) * g.Ws + c * g.abstand;
}

// The S domain pixels that the range pixels x0 .. x0 + S - 1 of pixel row ry are painted from under isometry k of side B
// (range pixel (rx, ry) takes the domain pixel at src_k(rx, ry)).  k = 0: S contiguous ints of the domain row;
// else the run starts at src_k(x0, ry) and steps by the isometry's x-increment -- along a row (mirrored or not), or, for the
// four transposing isometries, down or up a column of the scaled image, one int per domain row.
template <int B, int S>
__device__ __forceinline__ void rgb_domain_seg(const int32_t* __restrict__ scaled, const FicGeom& g, int gi, int k, int ry, int x0,
                                               int32_t (&dom)[S])
{
    if (k == 0) {
        __builtin_memcpy(dom, rgb_domain_row(scaled, g, gi, ry) + x0, 4 * S);
    } else {
        const int32_t* d0 = rgb_domain_row(scaled, g, gi, 0);
        int ax, bx_, cx, ay, by_, cy;
        iso_affine(k, B - 1, ax, bx_, cx, ay, by_, cy);
        const int sx = ay * g.Ws + ax, s0 = (cy + by_ * ry) * g.Ws + cx + bx_ * ry + sx * x0;
#pragma unroll
        for (int x = 0; x < S; x++) dom[x] = d0[s0 + sx * x];
    }
}

// The same over the channels R, G, B: q = {q1, q2, q3, q4}, k the block's isometry (the constant 0 for QtRgb).
template <int B>
__device__ __forceinline__ uint32_t qt_row_sse(const int32_t* __restrict__ prow, const int32_t* __restrict__ scaled, const FicGeom& g,
                                               int gi, int k, int ry, const int32_t* __restrict__ q)
{
    const FicRgbCoef cf = rgb_row_coef(q[0], q[1], q[2], q[3]);
    uint32_t s = 0;
    auto add = [&](int x, int32_t d) {
        int vR, vG, vB;
        rgb_paint_px(cf, d, vR, vG, vB);
        s += rgb_sq(prow[x], vR, vG, vB);
    };
    if (k == 0) {       // read straight from the row, not through rgb_domain_seg's copy: k_leaf_sse<QtRgb, B> keeps its instruction count
        const int32_t* drow = rgb_domain_row(scaled, g, gi, ry);
#pragma unroll
        for (int x = 0; x < B; x++) add(x, drow[x]);
    } else {
        int32_t dom[B];
        rgb_domain_seg<B, B>(scaled, g, gi, k, ry, 0, dom);
#pragma unroll
        for (int x = 0; x < B; x++) add(x, dom[x]);
    }
    return s;
}

// ---------------------------------------------------------------------------------------------
// k_leaf_sse<Fmt, B>: sse[j] = sum over the block's pixels (and channels) of (orig - value)^2, exact.  One thread per pixel row
// of a range block, ordered like k_decode_paint (block row, pixel row, block column); the B row sums of a block meet in sse[j]
// (zeroed by the launcher) through integer atomics, so the result does not depend on their order.  At most
// 256 * 3 * 255^2 < 2^32 per block.  A batch: blockIdx.y is the plane -- image [planes][H][W], scaled [planes][Hs][Ws], qrows
// [planes][Nr][QW], iso [planes][Nr], sse [planes][sse_stride]; the workgroups of a plane end with the plane, so none spans two.
// ---------------------------------------------------------------------------------------------
template <typename Fmt, int B>
__global__ __launch_bounds__(256) void k_leaf_sse(const typename Fmt::Px* __restrict__ image, const typename Fmt::Px* __restrict__ scaled,
                                                  const int32_t* __restrict__ qrows, const int32_t* __restrict__ iso,
                                                  uint32_t* __restrict__ sse, FicGeom g, size_t sse_stride)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= g.Nr * B) return;
    const size_t p = blockIdx.y;
    image += p * g.W * g.H;
    scaled += p * g.Ws * g.Hs;
    qrows += p * g.Nr * Fmt::QW;
    if (iso) iso += p * g.Nr;
    sse += p * sse_stride;
    const int bx = t % g.Rw, row = t / g.Rw;
    const int ry = row % B, by = row / B;
    const int j = by * g.Rw + bx;
    const int32_t* q = qrows + Fmt::QW * (size_t)j;
    const int wloc = q[0];
    const bool ok = wloc >= 0 && wloc < g.wK * g.wK;
    const int gi = ok ? window_to_global(g, j, wloc) : -1;
    if (gi < 0 || gi >= g.Nd) { atomicOr(&sse[j], 0xFFFFFFFFu); return; }   // never for an encoder's own rows: always split
    int k = 0;
    if constexpr (Fmt::kIso) k = iso ? iso[j] : 0;
    const uint32_t s = qt_row_sse<B>(image + (size_t)row * g.W + bx * B, scaled, g, gi, k, ry, q + 1);
    if (s) atomicAdd(&sse[j], s);
}

// ---------------------------------------------------------------------------------------------
// Split + compaction.  Level l = 0 .. nl-1 has block side B_max >> l; a block of level l is split iff l < nl - 1 and
// (double) sse_l > (double) threshold * B * B.  Leaves are visited depth first, children TL, TR, BL, BR, top-level blocks in
// scanline order.  One thread per top-level block walks its subtree (at most 1 + 4 + 16 nodes) with a small explicit stack:
// k_qt_count counts the leaves, k_qt_scan (one workgroup) turns the counts into offsets, k_qt_scatter walks again and writes
// the rows at its offset: {x, y, B} and the level's quantised row, {idx_local, qa, qb, iso} (grey) or {idx_local, q1, q2, q3,
// q4} (colour; QtRgbIso: + iso).
// ---------------------------------------------------------------------------------------------
// A batch of planes (blockIdx.y of the walkers and the key kernels): the arrays of plane p start p strides behind those of
// plane 0 -- sse_stride u32 for the SSE of every level, Nr[l] rows for qrows and iso -- and the threshold rule reads its
// threshold from thr[p] (device memory: put there by the host or left there by the budget's select).
struct FicQtLevels {
    const uint32_t* sse[3];
    const int32_t* qrows[3];     // QW ints per range block (k_qt_scatter)
    const int32_t* iso[3];       // NULL: n_iso = 1 (iso 0)
    int Rw[3];
    int Nr[3];                   // range blocks per plane and level
    int nl;                      // levels
    int B_max;
    int Rw_top, Ntop;
    int QW;                      // ints per row of qrows (0: none given)
    size_t sse_stride;
    const float* thr;            // [planes], the threshold rule's; NULL for the kernels that do not split by threshold
    float threshold;             // of the plane: qt_plane's copy of thr[p]
};

// Entry l of a per-level array by selection, not by address: the walkers' l is a run-time value, and the levels of a plane
// (qt_plane's copy) stay in registers only while nothing indexes them in memory.
template <typename T>
__device__ __forceinline__ T qt_lv(const T (&a)[3], int l) { return l == 0 ? a[0] : (l == 1 ? a[1] : a[2]); }

// The levels of plane p: what the per-block code below works on, whichever plane it is
__device__ __forceinline__ FicQtLevels qt_plane(FicQtLevels L, int p)
{
#pragma unroll
    for (int l = 0; l < 3; l++)
        if (l < L.nl) {
            L.sse[l] += (size_t)p * L.sse_stride;
            if (L.qrows[l]) L.qrows[l] += (size_t)p * L.Nr[l] * L.QW;
            if (L.iso[l]) L.iso[l] += (size_t)p * L.Nr[l];
        }
    if (L.thr) L.threshold = L.thr[p];
    return L;
}

__device__ __forceinline__ bool qt_split(const FicQtLevels& L, int l, int x, int y)
{
    if (l >= L.nl - 1) return false;
    const int B = L.B_max >> l;
    const uint32_t s = qt_lv(L.sse, l)[(y / B) * qt_lv(L.Rw, l) + x / B];
    return (double)s > (double)L.threshold * (double)B * (double)B;
}

// The split rules of the walkers: split(L, l, x, y) for the block of level l at pixel (x, y).  QtByThreshold: the rule above.
// QtByKey: a block above B_min splits iff its key e(v) > lambda; keys as k_qt_rd_keys writes them (level 0,
// then level 1), lambda read from device memory, where the select left it.
// at(p): the rule of plane p (keys [planes][nkeys], lambda [planes]; the threshold comes with qt_plane).
struct QtByThreshold {
    __device__ __forceinline__ QtByThreshold at(int) const { return *this; }
    __device__ __forceinline__ bool operator()(const FicQtLevels& L, int l, int x, int y) const { return qt_split(L, l, x, y); }
};
struct QtByKey {
    const uint32_t* keys;
    const uint32_t* lambda;
    int nkeys;
    __device__ __forceinline__ QtByKey at(int p) const { return QtByKey{keys + (size_t)p * nkeys, lambda + p, nkeys}; }
    __device__ __forceinline__ bool operator()(const FicQtLevels& L, int l, int x, int y) const
    {
        if (l >= L.nl - 1) return false;
        const int B = L.B_max >> l;
        return keys[(l ? L.Ntop : 0) + (y / B) * qt_lv(L.Rw, l) + x / B] > *lambda;
    }
};

// Walks the subtree of top-level block t in DFS order; emit(x, y, l) per leaf.
template <typename Split, typename F>
__device__ __forceinline__ void qt_walk(const FicQtLevels& L, const Split& split, int t, F emit)
{
    int sx[8], sy[8], sl[8];
    int sp = 0;
    sx[0] = (t % L.Rw_top) * L.B_max;
    sy[0] = (t / L.Rw_top) * L.B_max;
    sl[0] = 0;
    sp = 1;
    while (sp > 0) {
        sp--;
        const int x = sx[sp], y = sy[sp], l = sl[sp];
        if (split(L, l, x, y)) {
            const int h = (L.B_max >> l) / 2;       // children pushed BR, BL, TR, TL: popped TL first
            sx[sp] = x + h; sy[sp] = y + h; sl[sp] = l + 1; sp++;
            sx[sp] = x;     sy[sp] = y + h; sl[sp] = l + 1; sp++;
            sx[sp] = x + h; sy[sp] = y;     sl[sp] = l + 1; sp++;
            sx[sp] = x;     sy[sp] = y;     sl[sp] = l + 1; sp++;
        } else {
            emit(x, y, l);
        }
    }
}

template <typename Split>
__global__ __launch_bounds__(256) void k_qt_count(FicQtLevels L0, Split split0, int* __restrict__ counts)      // counts [planes][Ntop]
{
    const int t = blockIdx.x * 256 + threadIdx.x, p = blockIdx.y;
    if (t >= L0.Ntop) return;
    const FicQtLevels L = qt_plane(L0, p);
    const Split split = split0.at(p);
    int n = 0;
    qt_walk(L, split, t, [&](int, int, int) { n++; });
    counts[(size_t)p * L.Ntop + t] = n;
}

// Exclusive scan of counts[0 .. n) into offs[0 .. n), offs[n] = the total.  One workgroup: every thread sums a contiguous
// slice, the slice sums are scanned in LDS, then every thread writes its slice's offsets.  A batch: one workgroup per plane
// (blockIdx.x) on counts [planes][n] and offs [planes][n + 1]; totals [planes] gets every plane's total once more.
#define FIC_QT_SCAN_THREADS 1024
__global__ __launch_bounds__(FIC_QT_SCAN_THREADS) void k_qt_scan(const int* __restrict__ counts, int* __restrict__ offs, int n,
                                                                 int* __restrict__ totals)
{
    __shared__ int part[FIC_QT_SCAN_THREADS];
    const int t = threadIdx.x;
    counts += (size_t)blockIdx.x * n;
    offs += (size_t)blockIdx.x * (n + 1);
    const int per = (n + FIC_QT_SCAN_THREADS - 1) / FIC_QT_SCAN_THREADS;
    const int i0 = t * per, i1 = i0 + per < n ? i0 + per : n;
    int s = 0;
    for (int i = i0; i < i1; i++) s += counts[i];
    part[t] = s;
    __syncthreads();
    for (int stride = 1; stride < FIC_QT_SCAN_THREADS; stride <<= 1) {     // inclusive Hillis-Steele scan of the slice sums
        const int v = t >= stride ? part[t - stride] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int run = part[t] - s;
    for (int i = i0; i < i1; i++) {
        offs[i] = run;
        run += counts[i];
    }
    if (t == FIC_QT_SCAN_THREADS - 1) {
        offs[n] = part[t];
        totals[blockIdx.x] = part[t];
    }
}

// Leaf rows of Fmt::QW + 3 ints, formats with kIso one more: the iso column follows the quantised row
template <typename Fmt, typename Split>
__global__ __launch_bounds__(256) void k_qt_scatter(FicQtLevels L0, Split split0, const int* __restrict__ offs, int32_t* __restrict__ leaves,
                                                    size_t leaf_stride)      // offs [planes][Ntop + 1], leaves [planes][leaf_stride] ints
{
    constexpr int QW = Fmt::QW;
    const int t = blockIdx.x * 256 + threadIdx.x, p = blockIdx.y;
    if (t >= L0.Ntop) return;
    const FicQtLevels L = qt_plane(L0, p);
    const Split split = split0.at(p);
    leaves += (size_t)p * leaf_stride;
    int o = offs[(size_t)p * (L.Ntop + 1) + t];
    qt_walk(L, split, t, [&](int x, int y, int l) {
        const int B = L.B_max >> l;
        const int j = (y / B) * qt_lv(L.Rw, l) + x / B;
        const int32_t *rows = qt_lv(L.qrows, l), *isos = qt_lv(L.iso, l);
        int32_t* r = leaves + Fmt::kLeafInts * (size_t)o;
        r[0] = x;
        r[1] = y;
        r[2] = B;
#pragma unroll
        for (int k = 0; k < QW; k++) r[3 + k] = rows[QW * j + k];
        if constexpr (Fmt::kIso) r[3 + QW] = isos ? isos[j] : 0;
        o++;
    });
}

// ---------------------------------------------------------------------------------------------
// Encode to a leaf budget.  Block v of side B above B_min splits under threshold t iff (double) SSE_v >
// (double) t * B * B, that is iff k(v) = SSE_v * (256 / B^2) > 256 t: one denominator for every level (x1 at B = 16, x4 at
// B = 8; below 2^26 for an encoder's own rows, saturated at 2^32 - 1 for k_leaf_sse's all-ones mark).  v is reached only when
// every ancestor splits, so with e(v) = min(k(v), k(parent(v)), ..) the tree under t has Ntop + 3 #{v : e(v) > 256 t} leaves.
// k_qt_keys writes e(v), the blocks of level 0 first, then (three levels) those of level 1; one thread per block.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t qt_key(const FicQtLevels& L, int l, int j)
{
    const int B = L.B_max >> l;
    const unsigned long long k = (unsigned long long)L.sse[l][j] * (unsigned long long)(256 / (B * B));
    return k > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)k;
}

__global__ __launch_bounds__(256) void k_qt_keys(FicQtLevels L0, int n1, uint32_t* __restrict__ keys)      // keys [planes][Ntop + n1]
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    const FicQtLevels L = qt_plane(L0, blockIdx.y);
    keys += (size_t)blockIdx.y * (L.Ntop + n1);
    if (t < L.Ntop) {
        keys[t] = qt_key(L, 0, t);
    } else if (t < L.Ntop + n1) {
        const int j = t - L.Ntop, x = j % L.Rw[1], y = j / L.Rw[1];
        const uint32_t k = qt_key(L, 1, j), kp = qt_key(L, 0, (y / 2) * L.Rw[0] + x / 2);
        keys[t] = k < kp ? k : kp;
    }
}

// Radix select of the key of rank `rank` in descending order (rank 0: the largest), four passes of 8 bits from the top byte.
// bins u32 [4][256], zeroed by the launcher: bins[p] is the histogram of byte 3 - p over the keys whose higher bytes are the
// prefix chosen so far.  The keys are thought followed by endlessly many zeros, so a rank past the last key selects 0.
//
// qt_select_resolve: prefix and remaining rank after the first `npass` passes, from their final bins alone; every workgroup
// that needs them computes them again (256 values per pass; wave 0 holds four bins per lane and scans the lane sums from the
// top), so no state is written by more than one workgroup.  Per pass the digit d is the largest with #{digit >= d} > rem,
// 0 when there is none (the zeros behind the keys); rem then drops by #{digit > d}.  Called by all 256 threads.
__device__ __forceinline__ void qt_select_resolve(const uint32_t* __restrict__ bins, int npass, uint32_t rank, uint32_t& prefix, uint32_t& rem)
{
    __shared__ uint32_t s_prefix, s_rem;
    if (threadIdx.x == 0) { s_prefix = 0; s_rem = rank; }
    __syncthreads();
    for (int p = 0; p < npass; p++) {
        const uint32_t pre = s_prefix, r = s_rem;
        __syncthreads();
        if (threadIdx.x < 64) {
            const int lane = threadIdx.x;
            const uint4 b = *(const uint4*)(bins + 256 * p + 4 * lane);
            const uint32_t own = b.x + b.y + b.z + b.w;
            uint32_t incl = own;                            // keys of digit >= 4 lane
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t v = __shfl_down(incl, off, 64);
                if (lane + off < 64) incl += v;
            }
            const uint32_t above = incl - own;              // keys of digit >= 4 (lane + 1)
            if (above <= r && r < incl) {                   // one lane at most
                const uint32_t c3 = above + b.w, c2 = c3 + b.z, c1 = c2 + b.y;
                const int d = r < c3 ? 3 : (r < c2 ? 2 : (r < c1 ? 1 : 0));
                s_prefix = (pre << 8) | (uint32_t)(4 * lane + d);
                s_rem = r - (d == 3 ? above : (d == 2 ? c3 : (d == 1 ? c2 : c1)));
            } else if (lane == 0 && incl <= r) {            // fewer keys than the rank asks for: digit 0
                s_prefix = pre << 8;
                s_rem = r - (incl - b.x);
            }
        }
        __syncthreads();
    }
    prefix = s_prefix;
    rem = s_rem;
}

// One pass: 256 threads per workgroup with a grid stride over the keys, a 256-bin histogram in LDS, one global atomic per
// non-empty bin.
// A batch is P independent selects, blockIdx.y the plane: keys [planes][n], work [planes][FIC_QT_SELECT_WORDS] (bins, then the
// result), and the rank of plane p is ranks[p], read from device memory.
__global__ __launch_bounds__(256) void k_qt_select_hist(const uint32_t* __restrict__ keys, uint32_t n, const uint32_t* __restrict__ ranks,
                                                        uint32_t* __restrict__ work, int pass)
{
    __shared__ uint32_t hist[256];
    hist[threadIdx.x] = 0;
    keys += (size_t)blockIdx.y * n;
    uint32_t* bins = work + (size_t)blockIdx.y * FIC_QT_SELECT_WORDS;
    const uint32_t rank = ranks[blockIdx.y];
    uint32_t prefix, rem;
    qt_select_resolve(bins, pass, rank, prefix, rem);       // its barriers also cover hist's zeroes
    const int shift = 24 - 8 * pass;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const uint32_t k = keys[i];
        if (pass == 0 || (k >> (shift + 8)) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);
    }
    __syncthreads();
    const uint32_t c = hist[threadIdx.x];
    if (c) atomicAdd(&bins[256 * pass + threadIdx.x], c);
}

// One workgroup: resolves the last pass.  out = {K, the bits of the threshold, #{keys > K}, 0}; the threshold is the smallest
// float >= K / 256: K rounded up to a float, times 2^-8 (exact).
// One workgroup per plane (blockIdx.x); param [planes] gets word `param_word` of the plane's result: the rule's parameter.
__global__ __launch_bounds__(256) void k_qt_select_final(uint32_t* __restrict__ work, const uint32_t* __restrict__ ranks,
                                                         uint32_t* __restrict__ param, int param_word)
{
    const uint32_t* bins = work + (size_t)blockIdx.x * FIC_QT_SELECT_WORDS;
    uint32_t* out = work + (size_t)blockIdx.x * FIC_QT_SELECT_WORDS + 4 * 256;
    const uint32_t rank = ranks[blockIdx.x];
    uint32_t K, rem;
    qt_select_resolve(bins, 4, rank, K, rem);
    if (threadIdx.x == 0) {
        out[0] = K;
        out[1] = __float_as_uint(__fmul_rn(__uint2float_ru(K), 0x1p-8f));
        out[2] = rank - rem;
        out[3] = 0;
        param[blockIdx.x] = out[param_word];
    }
}

// stats u64 [4], zeroed by the launcher: the collage SSE summed over the leaves of the tree under the split rule, and its leaves
// of side B_max, B_max / 2, B_max / 4.  One thread per top-level block, k_qt_count's walk; wave sums, then one atomic per
// wave and non-zero value.
template <typename Split>
__global__ __launch_bounds__(256) void k_qt_tree_stats(FicQtLevels L0, Split split0, unsigned long long* __restrict__ stats)   // stats [planes][4]
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    const FicQtLevels L = qt_plane(L0, blockIdx.y);
    const Split split = split0.at(blockIdx.y);
    stats += 4 * (size_t)blockIdx.y;
    unsigned long long v[4] = {0, 0, 0, 0};
    if (t < L.Ntop)
        qt_walk(L, split, t, [&](int x, int y, int l) {
            const int B = L.B_max >> l;
            v[0] += qt_lv(L.sse, l)[(y / B) * qt_lv(L.Rw, l) + x / B];
            v[1 + l]++;
        });
#pragma unroll
    for (int i = 0; i < 4; i++) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v[i] += __shfl_xor(v[i], off, 64);
        if ((threadIdx.x & 63) == 0 && v[i]) atomicAdd(&stats[i], v[i]);
    }
}

// ---------------------------------------------------------------------------------------------
// Encode by rate-distortion pruning: the tree T(lambda) that minimises D + lambda N, D the summed SSE of the
// leaves and N their number, lambda an integer in 0 .. 2^32 - 1.  With S_v the u32 of k_leaf_sse widened to 64 bits, block v
// above B_min wants to split iff the cost of its children, sum of J(c), is < S_v + lambda, where J(c) = S_c + lambda at B_min and
// min(S_c + lambda, sum of J over c's children) above; k(v) is the smallest lambda >= 0 at which it does not:
//   children of side B_min:      k(v) = max(0, ceil((S_v - sum S_c) / 3))
//   top block of three levels:   the smallest lambda with f(lambda) = sum_c min(S_c + lambda, SS_c + 4 lambda) - S_v - lambda >= 0
//                                (SS_c the sum over c's children); f has slope >= 3 and f(ceil(S_v / 3)) >= 0, so a bisection
//                                over [0, ceil(S_v / 3)] finds it in at most 31 steps, and k(v) < 2^31
// e(v) = min(k(v), k(parent)) and G_v = S_v - sum S_c (signed).  All of it in int64: S <= 2^32 - 1, lambda < 2^31, so no term
// passes 2^37.  One thread per block above B_min in the order of k_qt_keys; a thread of level 1 works its parent's k out again
// (21 loads) instead of waiting for it.  *top_sum (zeroed by the launcher) += the sum of S over the top-level blocks.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ long long qt_child_sum(const FicQtLevels& L, int l, int j)
{
    const int x = j % L.Rw[l], y = j / L.Rw[l], Rc = L.Rw[l + 1];
    const uint32_t* c = L.sse[l + 1] + (size_t)(2 * y) * Rc + 2 * x;
    return (long long)c[0] + (long long)c[1] + (long long)c[Rc] + (long long)c[Rc + 1];
}

__device__ __forceinline__ uint32_t qt_rd_k_last(long long S, long long kids)
{
    const long long g = S - kids;
    return g <= 0 ? 0u : (uint32_t)((g + 2) / 3);
}

__device__ __forceinline__ uint32_t qt_rd_k_top(const FicQtLevels& L, int j)      // three levels, j a block of level 0
{
    const long long S = L.sse[0][j];
    const int x = j % L.Rw[0], y = j / L.Rw[0];
    long long sc[4], scc[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const int jc = (2 * y + (c >> 1)) * L.Rw[1] + 2 * x + (c & 1);
        sc[c] = L.sse[1][jc];
        scc[c] = qt_child_sum(L, 1, jc);
    }
    auto f = [&](long long lam) {
        long long s = -S - lam;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const long long whole = sc[c] + lam, parts = scc[c] + 4 * lam;
            s += whole < parts ? whole : parts;
        }
        return s;
    };
    if (f(0) >= 0) return 0u;
    long long lo = 0, hi = (S + 2) / 3;             // f(lo) < 0 <= f(hi)
    while (hi - lo > 1) {
        const long long mid = (lo + hi) >> 1;
        if (f(mid) >= 0) hi = mid;
        else lo = mid;
    }
    return (uint32_t)hi;
}

__global__ __launch_bounds__(256) void k_qt_rd_keys(FicQtLevels L0, int n1, uint32_t* __restrict__ keys, long long* __restrict__ gains,
                                                    unsigned long long* __restrict__ top_sum)   // keys, gains [planes][Ntop + n1], top_sum [planes]
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    const FicQtLevels L = qt_plane(L0, blockIdx.y);
    keys += (size_t)blockIdx.y * (L.Ntop + n1);
    gains += (size_t)blockIdx.y * (L.Ntop + n1);
    top_sum += blockIdx.y;
    unsigned long long s_top = 0;
    if (t < L.Ntop) {
        const long long S = L.sse[0][t], kids = qt_child_sum(L, 0, t);
        keys[t] = L.nl == 3 ? qt_rd_k_top(L, t) : qt_rd_k_last(S, kids);
        gains[t] = S - kids;
        s_top = (unsigned long long)S;
    } else if (t < L.Ntop + n1) {
        const int j = t - L.Ntop, x = j % L.Rw[1], y = j / L.Rw[1];
        const long long S = L.sse[1][j], kids = qt_child_sum(L, 1, j);
        const uint32_t k = qt_rd_k_last(S, kids), kp = qt_rd_k_top(L, (y / 2) * L.Rw[0] + x / 2);
        keys[t] = k < kp ? k : kp;
        gains[t] = S - kids;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s_top += __shfl_xor(s_top, off, 64);
    if ((threadIdx.x & 63) == 0 && s_top) atomicAdd(top_sum, s_top);
}

// The weighted select: with A(x) = the sum of gain over the keys > x, the largest b among the keys and 0 with A(b) >= need, or
// 0 when there is none.  Precondition: A is non-increasing in x (the summed gain over descending distinct keys never falls).
// Then "A(x) < need" is monotone in x, and x0 = min{x : A(x) < need} (2^32 when there is none, i.e. need <= 0) comes out of
// the radix select of 4.18 with int64 gain sums in the bins: per pass, with `acc` the gain above the prefix, the digit is the
// smallest d with acc + #{gain of digits > d} < need -- every larger digit passes too, none smaller does -- and acc grows by
// that sum.  x0 is a key or 0, and b = the largest key < x0.  need = (int64) *total - value, both on the device (an SSE target:
// the top-level sum minus max_sse).
//
// qt_select_w_resolve: x0's prefix and acc after `npass` passes from their final bins (i64 [4][256]), by all 256 threads: an
// inclusive suffix scan of the pass's 256 sums in LDS, then the smallest passing digit through an LDS atomicMin.
__device__ __forceinline__ void qt_select_w_resolve(const long long* __restrict__ bins, int npass, long long need, uint32_t& prefix,
                                                    bool& none)
{
    __shared__ long long s_suf[256];
    __shared__ long long s_acc;
    __shared__ uint32_t s_prefix;
    __shared__ int s_d;
    const int tid = threadIdx.x;
    if (tid == 0) { s_prefix = 0; s_acc = 0; }
    none = false;
    for (int p = 0; p < npass; p++) {
        __syncthreads();
        const uint32_t pre = s_prefix;
        const long long acc = s_acc, own = bins[256 * p + tid];
        s_suf[tid] = own;
        if (tid == 0) s_d = 256;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            const long long v = tid + off < 256 ? s_suf[tid + off] : 0;
            __syncthreads();
            s_suf[tid] += v;
            __syncthreads();
        }
        const long long above = s_suf[tid] - own;       // the gain of the digits > tid
        if (acc + above < need) atomicMin(&s_d, tid);
        __syncthreads();
        const int d = s_d;                              // uniform
        if (d == 256) { none = true; break; }           // pass 0 only: later, digit 255 passes by the choice before it
        if (tid == d) { s_prefix = (pre << 8) | (uint32_t)d; s_acc = acc + above; }
    }
    __syncthreads();
    prefix = s_prefix;
}

// One pass: k_qt_select_hist with the gains summed per bin (64-bit LDS adds, one global atomic per bin with a non-zero sum).
// A batch, as k_qt_select_hist: blockIdx.y the plane, keys and gains [planes][n], total and values [planes], work [planes]
// [FIC_QT_SELECT_W_WORDS].
__global__ __launch_bounds__(256) void k_qt_select_hist_w(const uint32_t* __restrict__ keys, const long long* __restrict__ gains, uint32_t n,
                                                          const unsigned long long* __restrict__ total, const long long* __restrict__ values,
                                                          long long* __restrict__ work, int pass)
{
    __shared__ unsigned long long hist[256];
    hist[threadIdx.x] = 0;
    keys += (size_t)blockIdx.y * n;
    gains += (size_t)blockIdx.y * n;
    const long long need = (long long)total[blockIdx.y] - values[blockIdx.y];
    long long* bins = work + (size_t)blockIdx.y * FIC_QT_SELECT_W_WORDS;
    uint32_t prefix;
    bool none;
    qt_select_w_resolve(bins, pass, need, prefix, none);                                // its barriers also cover hist's zeroes
    if (none) return;                                                                   // uniform
    const int shift = 24 - 8 * pass;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const uint32_t k = keys[i];
        if (pass == 0 || (k >> (shift + 8)) == prefix) atomicAdd(&hist[(k >> shift) & 255u], (unsigned long long)gains[i]);
    }
    __syncthreads();
    const unsigned long long c = hist[threadIdx.x];
    if (c) atomicAdd((unsigned long long*)&bins[256 * pass + threadIdx.x], c);
}

// The last step, again over all keys: out u64 [4], zeroed by the launcher = {b in the low 32 bits, #{keys > b}, the sum of
// their gains (signed), 0}.  b = max{key < x0} or 0; the keys > b are those >= max(x0, 1).  Wave sums, then one atomic
// each per wave and non-zero value.
// param (u32 [planes], zeroed by the launcher) gets every plane's b once more: the lambda its walkers read.
__global__ __launch_bounds__(256) void k_qt_select_final_w(const uint32_t* __restrict__ keys, const long long* __restrict__ gains, uint32_t n,
                                                           const unsigned long long* __restrict__ total, const long long* __restrict__ values,
                                                           unsigned long long* __restrict__ work, uint32_t* __restrict__ param)
{
    keys += (size_t)blockIdx.y * n;
    gains += (size_t)blockIdx.y * n;
    const long long need = (long long)total[blockIdx.y] - values[blockIdx.y];
    const long long* bins = (const long long*)work + (size_t)blockIdx.y * FIC_QT_SELECT_W_WORDS;
    unsigned long long* out = work + (size_t)blockIdx.y * FIC_QT_SELECT_W_WORDS + 4 * 256;
    uint32_t prefix;
    bool none;
    qt_select_w_resolve(bins, 4, need, prefix, none);
    const unsigned long long x0 = none ? 0x100000000ull : (unsigned long long)prefix, from = x0 ? x0 : 1ull;
    uint32_t b = 0;
    unsigned long long cnt = 0, gain = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const uint32_t k = keys[i];
        if (k < x0 && k > b) b = k;
        if (k >= from) { cnt++; gain += (unsigned long long)gains[i]; }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t ob = __shfl_xor(b, off, 64);
        b = ob > b ? ob : b;
        cnt += __shfl_xor(cnt, off, 64);
        gain += __shfl_xor(gain, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (b) atomicMax((uint32_t*)out, b);
        if (b) atomicMax(param + blockIdx.y, b);
        if (cnt) atomicAdd(out + 1, cnt);
        if (gain) atomicAdd(out + 2, gain);
    }
}

// ---------------------------------------------------------------------------------------------
// One segment -- S pixels from x0 on; the whole row up to B = 16 -- of pixel row ry of one decoder paint of leaf e, grey
// (FC:385-407): paints prow, stores the squared changes to srow (both at the segment), returns their sum.
// ---------------------------------------------------------------------------------------------
template <int B, int S>
__device__ __forceinline__ uint32_t qt_paint_row(uint8_t* __restrict__ prow, uint32_t* __restrict__ srow, const uint8_t* __restrict__ scaled,
                                                 const FicGeom& g, const FicQtLeaf& e, int ry, int x0)
{
    uint32_t old[S / 4], neu[S / 4], sqv[S], sq = 0;
    __builtin_memcpy(old, prow, S);
    int value[S];
    qt_row_values<B, S>(scaled, g, e.gi, e.q[2], ry, x0, __fdiv_rn((float)e.q[0], 100.0f), (float)e.q[1], value);
#pragma unroll
    for (int q = 0; q < S / 4; q++) neu[q] = 0u;
#pragma unroll
    for (int x = 0; x < S; x++) {
        const int dd = (int)((old[x >> 2] >> (8 * (x & 3))) & 0xffu) - value[x];
        neu[x >> 2] |= (uint32_t)value[x] << (8 * (x & 3));
        sqv[x] = (uint32_t)(dd * dd);
        sq += sqv[x];
    }
    __builtin_memcpy(prow, neu, S);
#pragma unroll
    for (int q = 0; q < S / 4; q++) *(uint4*)(srow + 4 * q) = make_uint4(sqv[4 * q], sqv[4 * q + 1], sqv[4 * q + 2], sqv[4 * q + 3]);
    return sq;
}

// The same for decodeRGB (FC:458-499): the squares are dR^2 + dG^2 + dB^2 per pixel (FC:493).  Leaf: FicQtLeaf (isometry 0)
// or FicQtLeafIso (the leaf's own).
__device__ __forceinline__ int qt_leaf_iso(const FicQtLeaf&) { return 0; }
__device__ __forceinline__ int qt_leaf_iso(const FicQtLeafIso& e) { return e.k; }
template <int B, int S, typename Leaf>
__device__ __forceinline__ uint32_t qt_paint_row(int32_t* __restrict__ prow, uint32_t* __restrict__ srow, const int32_t* __restrict__ scaled,
                                                 const FicGeom& g, const Leaf& e, int ry, int x0)
{
    const FicRgbCoef cf = rgb_row_coef(e.q[0], e.q[1], e.q[2], e.q[3]);
    int32_t cur[S], dom[S];
    uint32_t sqv[S], sq = 0;
    __builtin_memcpy(cur, prow, 4 * S);
    rgb_domain_seg<B, S>(scaled, g, e.gi, qt_leaf_iso(e), ry, x0, dom);
#pragma unroll
    for (int x = 0; x < S; x++) {
        int vR, vG, vB;
        rgb_paint_px(cf, dom[x], vR, vG, vB);
        sqv[x] = rgb_sq(cur[x], vR, vG, vB);
        sq += sqv[x];
        cur[x] = (int32_t)(0xff000000u | ((uint32_t)vR << 16) | ((uint32_t)vG << 8) | (uint32_t)vB);
    }
    __builtin_memcpy(prow, cur, 4 * S);
    __builtin_memcpy(srow, sqv, 4 * S);
    return sq;
}

// Adds the workgroup's (256 threads) sum of sq to *ssd: wave reduction, then one atomic per workgroup.
__device__ __forceinline__ void qt_ssd_add(unsigned long long sq, unsigned long long* ssd)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sq += __shfl_xor(sq, off, 64);
    __shared__ unsigned long long s_part[4];
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = sq;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long tot = s_part[0] + s_part[1] + s_part[2] + s_part[3];
        if (tot) atomicAdd(ssd, tot);
    }
}

// ---------------------------------------------------------------------------------------------
// k_decode_paint_leaves<Fmt, B>: one decoder paint of the n leaves of side B in `lv`.  Each entry carries the leaf's position,
// its global domain block (window_to_global of its level, resolved by the reader), its offset in `sqbuf` (the prefix sum of
// B^2 over the leaves before it, so the squares lie in leaf order, pixel rows within a leaf) and its row.  One thread per pixel
// row of a leaf up to B = 16; at the decode-only sides 32 and 64 (zoomed decodes) per row SEGMENT of 16 grey or
// 4 packed ARGB pixels (16 bytes of the image per thread either way, a whole row would not fit a thread's registers), ordered
// (leaf, pixel row, segment): neighbours in a wave touch neighbouring bytes of the same image row.  The exact integer sum of
// the squares goes to state->ssd[counter] like k_decode_paint's.  Under an isometry (QtRgbIso) a thread's 4-pixel segment reads
// a run of 4 domain pixels from src_k(x0, ry) on, in the isometry's x direction (rgb_domain_seg).
// ---------------------------------------------------------------------------------------------
template <typename Fmt, int B>
constexpr int qt_paint_seg() { return B <= 16 ? B : (sizeof(typename Fmt::Px) == 1 ? 16 : 4); }
template <typename Fmt, int B>
__global__ __launch_bounds__(256) void k_decode_paint_leaves(const typename Fmt::Px* __restrict__ scaled, typename Fmt::Px* __restrict__ image,
                                                             const typename Fmt::Leaf* __restrict__ lv, int n, FicDecodeState* __restrict__ state,
                                                             uint32_t* __restrict__ sqbuf, int counter, FicGeom g)
{
    FicDecodeState* st = state;
    if (st->done) return;                                  // uniform
    const int t = blockIdx.x * 256 + threadIdx.x;
    unsigned long long sq = 0;
    constexpr int S = qt_paint_seg<Fmt, B>(), NS = B / S;
    if (t < n * B * NS) {
        const int x0 = (t % NS) * S, u = t / NS;
        const typename Fmt::Leaf e = lv[u / B];
        const int ry = u % B;
        sq = qt_paint_row<B, S>(image + (size_t)(e.y + ry) * g.W + e.x + x0, sqbuf + (size_t)e.sqoff + (size_t)ry * B + x0, scaled, g, e,
                                ry, x0);
    }
    qt_ssd_add(sq, &st->ssd[counter]);
}

// ---------------------------------------------------------------------------------------------
// Decode and collage of a batch straight from the encoder's leaf table: rows {x, y, B, idx_local, q.., iso} in
// stream order, leaves [planes][leaf_stride] ints, n_leaves [planes], both where the caller can write them.
//
// k_qt_resolve<Fmt>: one thread per leaf of a plane (blockIdx.y).  It checks the row before any address is formed from it -- the
// side in the ladder, x and y multiples of the side inside the image, idx_local inside the level's window, the isometry below
// n_iso, the domain block inside the level's pool, 1 <= n_leaves <= Nr_min -- writes the resolved entry (QtEntryWord,
// fic_qt_decode_plan.h: the stream decoder's leaf at the decode's zoom, sqoff from the closed form qt_decode_sqoff) and claims
// the leaf's (B / B_min)^2 cells of side B_min in the plane's cell map (filled with -1 by the launcher) with the leaf's index.
// A failed check or a cell that is taken already marks state[p].bad_index; the cells a plane's leaves did claim are counted in
// cover[p] (zeroed by the launcher), and k_qt_paint_planes paints a plane only if nothing is marked and cover[p] == Nr_min:
// every cell then belongs to exactly one leaf that passed every check and whose entry was written by this launch.
// ---------------------------------------------------------------------------------------------
template <typename Fmt>
__global__ __launch_bounds__(256) void k_qt_resolve(const int32_t* __restrict__ leaves, const int* __restrict__ n_leaves, FicQtDecode D,
                                                    int32_t* __restrict__ entries, int32_t* __restrict__ cells, int32_t* __restrict__ cover,
                                                    FicDecodeState* __restrict__ state)
{
    const int p = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    FicDecodeState* st = state + p;
    const int n = n_leaves[p];
    if (n < 1 || n > D.Nr_min) {                            // uniform per plane
        if (i == 0) st->bad_index = 1;
        return;
    }
    int claimed = 0;
    if (i < n) {
        const int32_t* r = leaves + (size_t)p * D.leaf_stride + (size_t)i * Fmt::kLeafInts;
        const int x = r[0], y = r[1], B = r[2], idx = r[3];
        int iso = 0;
        if constexpr (Fmt::kIso) iso = r[3 + Fmt::QW];
        int l = -1;
#pragma unroll
        for (int v = 0; v < 3; v++)
            if (v < D.nl && B == (D.B_max >> v)) l = v;
        bool ok = l >= 0;
        // W and H are multiples of B_max: a multiple of B below W leaves room for the whole leaf
        ok = ok && x >= 0 && y >= 0 && x < D.W && y < D.H && (x % B) == 0 && (y % B) == 0;
        int gi = -1;
        const FicGeom g = qt_lv(D.g, ok ? l : 0);           // the level at the decode's zoom: the block counts of the encode
        if (ok) {
            ok = idx >= 0 && idx < g.wK * g.wK && iso >= 0 && iso < D.n_iso;
            if (ok) gi = window_to_global(g, (y / B) * g.Rw + x / B, idx);
            ok = ok && gi >= 0 && gi < g.Nd;
        }
        if (ok) {
            const int nb = B / D.B_min, c0 = (y / D.B_min) * D.Rw_min + x / D.B_min;
            int32_t* cp = cells + (size_t)p * D.Nr_min;
            for (int cy = 0; cy < nb; cy++)
                for (int cx = 0; cx < nb; cx++) {
                    if (atomicCAS(&cp[c0 + cy * D.Rw_min + cx], -1, i) == -1) claimed++;
                    else ok = false;
                }
        }
        if (ok) {
            int4* e = (int4*)(entries + ((size_t)p * D.Nr_min + i) * kQtEntryInts);
            const int sqoff = (int)qt_decode_sqoff(x, y, B, D.B_max, D.Rw_top, D.zoom);
            int4 q;
            if constexpr (Fmt::QW == 3) q = make_int4(r[4], r[5], iso, 0);
            else q = make_int4(r[4], r[5], r[6], r[7]);
            e[0] = make_int4(D.zoom * x, D.zoom * y, gi, sqoff);
            e[1] = q;
            e[2] = make_int4(iso, D.zoom * B, 0, 0);
        } else {
            st->bad_index = 1;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) claimed += __shfl_xor(claimed, off, 64);
    if ((threadIdx.x & 63) == 0 && claimed) atomicAdd(&cover[p], claimed);
}

// The collage of one segment: the values of the quantised row from the scaled copy of the input, nothing read from the image
// and no squares -- the arithmetic k_leaf_sse sums, through the same functions.
template <int B, int S>
__device__ __forceinline__ void qt_collage_row(uint8_t* __restrict__ prow, const uint8_t* __restrict__ scaled, const FicGeom& g,
                                               const FicQtLeaf& e, int ry, int x0)
{
    int value[S];
    qt_row_values<B, S>(scaled, g, e.gi, e.q[2], ry, x0, __fdiv_rn((float)e.q[0], 100.0f), (float)e.q[1], value);
    uint32_t neu[S / 4];
#pragma unroll
    for (int q = 0; q < S / 4; q++) neu[q] = 0u;
#pragma unroll
    for (int x = 0; x < S; x++) neu[x >> 2] |= (uint32_t)value[x] << (8 * (x & 3));
    __builtin_memcpy(prow, neu, S);
}
template <int B, int S, typename Leaf>
__device__ __forceinline__ void qt_collage_row(int32_t* __restrict__ prow, const int32_t* __restrict__ scaled, const FicGeom& g,
                                               const Leaf& e, int ry, int x0)
{
    const FicRgbCoef cf = rgb_row_coef(e.q[0], e.q[1], e.q[2], e.q[3]);
    int32_t cur[S], dom[S];
    rgb_domain_seg<B, S>(scaled, g, e.gi, qt_leaf_iso(e), ry, x0, dom);
#pragma unroll
    for (int x = 0; x < S; x++) {
        int vR, vG, vB;
        rgb_paint_px(cf, dom[x], vR, vG, vB);
        cur[x] = (int32_t)(0xff000000u | ((uint32_t)vR << 16) | ((uint32_t)vG << 8) | (uint32_t)vB);
    }
    __builtin_memcpy(prow, cur, 4 * S);
}

// One segment of a leaf of side B through the row code above (qt_paint_row / qt_collage_row): the sum of its squares, 0 for the
// collage.  A segment is never wider than its leaf (S <= zoom B_min).
template <int B, int S, bool kCollage, typename Px, typename Leaf>
__device__ __forceinline__ uint32_t qt_plane_seg(Px* __restrict__ prow, uint32_t* __restrict__ srow, const Px* __restrict__ scaled,
                                                 const FicGeom& g, const Leaf& e, int ry, int x0)
{
    if constexpr (S > B) {
        return 0;
    } else if constexpr (kCollage) {
        qt_collage_row<B, S>(prow, scaled, g, e, ry, x0);
        return 0;
    } else {
        return qt_paint_row<B, S>(prow, srow, scaled, g, e, ry, x0);
    }
}

// ---------------------------------------------------------------------------------------------
// k_qt_paint_planes<Fmt, S, kCollage>: one decoder paint of every leaf of every plane (blockIdx.y), pixel-centric.  One thread
// per image segment of S pixels, threads in image order (row, segment): a wave writes consecutive bytes of the image.  S is 4
// packed ARGB pixels, or min(16, zoom B_min) grey ones (16 bytes, or the 4 / 8 that a cell of side zoom B_min = 4 / 8 holds), so
// a segment never leaves its cell, and the cell map names its leaf.  The squares go to sqbuf at the leaf's offset (Java's order:
// leaf by leaf, pixel rows within a leaf), the plane's exact sum to state[p].ssd[counter] as in k_decode_paint_leaves.  The
// row code is the stream decoder's, dispatched on the leaf's side: the lanes of a wave whose leaves differ in side take their
// case in turn (an image has at most three sides).
// kCollage: the one paint of the collage -- `scaled` is the 2:1 copy of the input, the image is only written, no squares.
// zW, zH: the image at the decode's zoom; cs = zoom B_min; scaled [planes][zH / 2][zW / 2]; Dw[l]: domain blocks per row of the
// level of side B_max >> l.
// ---------------------------------------------------------------------------------------------
struct FicQtPaint {
    int zW, zH, cs, Rw_min, Nr_min;
    int zB_max;              // zoom B_max
    int Dw[3];
};
template <typename Fmt, int S, bool kCollage>
__global__ __launch_bounds__(256) void k_qt_paint_planes(const typename Fmt::Px* __restrict__ scaled, typename Fmt::Px* __restrict__ image,
                                                         const int32_t* __restrict__ entries, const int32_t* __restrict__ cells,
                                                         const int32_t* __restrict__ cover, FicDecodeState* __restrict__ state,
                                                         uint32_t* __restrict__ sqbuf, int counter, FicQtPaint A)
{
    using Px = typename Fmt::Px;
    const int p = blockIdx.y;
    FicDecodeState* st = state + p;
    if (st->done || st->bad_index) return;                 // uniform per plane: a finished or refused plane is not touched
    if (cover[p] != A.Nr_min) {                            // (uniform) the leaves do not tile the image
        if (threadIdx.x == 0) st->bad_index = 1;
        return;
    }
    const int segs = A.zW / S, t = blockIdx.x * 256 + threadIdx.x;
    uint32_t sq = 0;
    if (t < segs * A.zH) {
        const int px = (t % segs) * S, py = t / segs;
        const int i = cells[(size_t)p * A.Nr_min + (py / A.cs) * A.Rw_min + px / A.cs];
        const int4* ep = (const int4*)(entries + ((size_t)p * A.Nr_min + i) * kQtEntryInts);
        const int4 e0 = ep[0], e1 = ep[1], e2 = ep[2];
        typename Fmt::Leaf e;
        e.x = e0.x; e.y = e0.y; e.gi = e0.z; e.sqoff = e0.w;
        e.q[0] = e1.x; e.q[1] = e1.y; e.q[2] = e1.z; e.q[3] = e1.w;
        if constexpr (sizeof(e) > sizeof(FicQtLeaf)) e.k = e2.x;
        const int side = e2.y, ry = py - e.y, x0 = px - e.x;
        FicGeom g{};                                       // what the row code takes from a level's geometry
        g.Ws = A.zW / 2;
        g.Dw = side == A.zB_max ? A.Dw[0] : (2 * side == A.zB_max ? A.Dw[1] : A.Dw[2]);
        g.abstand = side / 4;
        const size_t npix = (size_t)A.zW * A.zH;
        Px* prow = image + p * npix + (size_t)py * A.zW + px;
        uint32_t* srow = kCollage ? nullptr : sqbuf + p * npix + (size_t)e.sqoff + (size_t)ry * side + x0;
        const Px* sc = scaled + p * (npix / 4);
        switch (side) {
        case 4: sq = qt_plane_seg<4, S, kCollage>(prow, srow, sc, g, e, ry, x0); break;
        case 8: sq = qt_plane_seg<8, S, kCollage>(prow, srow, sc, g, e, ry, x0); break;
        case 16: sq = qt_plane_seg<16, S, kCollage>(prow, srow, sc, g, e, ry, x0); break;
        case 32: sq = qt_plane_seg<32, S, kCollage>(prow, srow, sc, g, e, ry, x0); break;
        default: sq = qt_plane_seg<64, S, kCollage>(prow, srow, sc, g, e, ry, x0); break;
        }
    }
    if constexpr (!kCollage) qt_ssd_add(sq, &st->ssd[counter]);
}

// ---------------------------------------------------------------------------------------------
// host-side launchers
// ---------------------------------------------------------------------------------------------
template <typename Fmt>
int fic_launch_leaf_sse(const typename Fmt::Px* image, const typename Fmt::Px* scaled, const int32_t* qrows, const int32_t* iso,
                        uint32_t* sse, const FicGeom& g, hipStream_t s, const FicQtPlanes& P)
{
    if (hipMemset2DAsync(sse, P.sse_stride * sizeof(uint32_t), 0, (size_t)g.Nr * sizeof(uint32_t), (size_t)P.planes, s) != hipSuccess) return -1;
    auto k = g.B == 4 ? k_leaf_sse<Fmt, 4> : (g.B == 8 ? k_leaf_sse<Fmt, 8> : k_leaf_sse<Fmt, 16>);
    hipLaunchKernelGGL(k, dim3((g.Nr * g.B + 255) / 256, P.planes), dim3(256), 0, s, image, scaled, qrows, iso, sse, g, P.sse_stride);
    FIC_LAUNCH_CHECK();
    return 0;
}

// qrows / iso NULL: for the kernels that read the SSE alone.  P: the strides of the batch and, for the threshold rule
// (by_threshold), its thresholds: P.param as floats
static FicQtLevels qt_levels_arg(const uint32_t* const* sse, const int32_t* const* qrows, const int32_t* const* iso, const int* Rw, int nl,
                                 int B_max, int Rw_top, int Ntop, int QW, const FicQtPlanes& P, bool by_threshold)
{
    FicQtLevels L{};
    for (int l = 0; l < nl; l++) {
        L.sse[l] = sse[l];
        L.qrows[l] = qrows ? qrows[l] : nullptr;
        L.iso[l] = iso ? iso[l] : nullptr;
        L.Rw[l] = Rw[l];
        L.Nr[l] = P.Nr[l];
    }
    L.nl = nl;
    L.B_max = B_max;
    L.Rw_top = Rw_top;
    L.Ntop = Ntop;
    L.QW = qrows ? QW : 0;
    L.sse_stride = P.sse_stride;
    L.thr = by_threshold ? (const float*)P.param : nullptr;
    return L;
}

int fic_launch_qt_keys(const uint32_t* const* sse, const int* Rw, int nl, int B_max, int Rw_top, int Ntop, int n1, uint32_t* keys,
                       hipStream_t s, const FicQtPlanes& P)
{
    const FicQtLevels L = qt_levels_arg(sse, nullptr, nullptr, Rw, nl, B_max, Rw_top, Ntop, 0, P, false);
    hipLaunchKernelGGL(k_qt_keys, dim3((Ntop + n1 + 255) / 256, P.planes), dim3(256), 0, s, L, n1, keys);
    FIC_LAUNCH_CHECK();
    return 0;
}

int fic_launch_qt_select(const uint32_t* keys, uint32_t n, uint32_t* work, hipStream_t s, const FicQtPlanes& P, int param_word)
{
    if (hipMemsetAsync(work, 0, (size_t)P.planes * FIC_QT_SELECT_WORDS * sizeof(uint32_t), s) != hipSuccess) return -1;
    const uint32_t need = (n + 255u) / 256u, nb = need < 1024u ? (need ? need : 1u) : 1024u;      // beyond: the grid stride
    for (int pass = 0; pass < 4; pass++) {
        hipLaunchKernelGGL(k_qt_select_hist, dim3(nb, P.planes), dim3(256), 0, s, keys, n, P.ranks, work, pass);
        FIC_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_qt_select_final, dim3(P.planes), dim3(256), 0, s, work, P.ranks, P.param, param_word);
    FIC_LAUNCH_CHECK();
    return 0;
}

template <typename Split>
static int qt_tree_stats(const FicQtLevels& L, const Split& split, unsigned long long* stats, hipStream_t s, int planes)
{
    if (hipMemsetAsync(stats, 0, (size_t)planes * 4 * sizeof(unsigned long long), s) != hipSuccess) return -1;
    hipLaunchKernelGGL(k_qt_tree_stats<Split>, dim3((L.Ntop + 255) / 256, planes), dim3(256), 0, s, L, split, stats);
    FIC_LAUNCH_CHECK();
    return 0;
}

int fic_launch_qt_tree_stats(const uint32_t* const* sse, const int* Rw, int nl, int B_max, int Rw_top, int Ntop,
                             unsigned long long* stats, hipStream_t s, const FicQtPlanes& P)
{
    return qt_tree_stats(qt_levels_arg(sse, nullptr, nullptr, Rw, nl, B_max, Rw_top, Ntop, 0, P, true), QtByThreshold{}, stats, s, P.planes);
}

int fic_launch_qt_tree_stats_rd(const uint32_t* const* sse, const int* Rw, int nl, int B_max, int Rw_top, int Ntop, const uint32_t* keys,
                                const uint32_t* lambda, unsigned long long* stats, hipStream_t s, const FicQtPlanes& P)
{
    return qt_tree_stats(qt_levels_arg(sse, nullptr, nullptr, Rw, nl, B_max, Rw_top, Ntop, 0, P, false), QtByKey{keys, lambda, P.nkeys}, stats, s, P.planes);
}

template <typename Fmt, typename Split>
static int qt_compact(const FicQtLevels& L, const Split& split, int* counts, int* offs, int32_t* leaves, hipStream_t s, const FicQtPlanes& P)
{
    const int nb = (L.Ntop + 255) / 256;
    hipLaunchKernelGGL(k_qt_count<Split>, dim3(nb, P.planes), dim3(256), 0, s, L, split, counts);
    FIC_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_qt_scan, dim3(P.planes), dim3(FIC_QT_SCAN_THREADS), 0, s, (const int*)counts, offs, L.Ntop, P.n_leaves);
    FIC_LAUNCH_CHECK();
    if (leaves) {
        hipLaunchKernelGGL((k_qt_scatter<Fmt, Split>), dim3(nb, P.planes), dim3(256), 0, s, L, split, (const int*)offs, leaves, P.leaf_stride);
        FIC_LAUNCH_CHECK();
    }
    return 0;
}

template <typename Fmt>
int fic_launch_qt_compact(const uint32_t* const* sse, const int32_t* const* qrows, const int32_t* const* iso, const int* Rw,
                          int nl, int B_max, int Rw_top, int Ntop, int* counts, int* offs, int32_t* leaves, hipStream_t s,
                          const FicQtPlanes& P)
{
    return qt_compact<Fmt>(qt_levels_arg(sse, qrows, iso, Rw, nl, B_max, Rw_top, Ntop, Fmt::QW, P, true), QtByThreshold{}, counts, offs, leaves, s, P);
}

template <typename Fmt>
int fic_launch_qt_compact_rd(const uint32_t* const* sse, const int32_t* const* qrows, const int32_t* const* iso, const int* Rw,
                             int nl, int B_max, int Rw_top, int Ntop, const uint32_t* keys, const uint32_t* lambda, int* counts,
                             int* offs, int32_t* leaves, hipStream_t s, const FicQtPlanes& P)
{
    return qt_compact<Fmt>(qt_levels_arg(sse, qrows, iso, Rw, nl, B_max, Rw_top, Ntop, Fmt::QW, P, false), QtByKey{keys, lambda, P.nkeys}, counts, offs,
                           leaves, s, P);
}

int fic_launch_qt_rd_keys(const uint32_t* const* sse, const int* Rw, int nl, int B_max, int Rw_top, int Ntop, int n1, uint32_t* keys,
                          long long* gains, unsigned long long* top_sum, hipStream_t s, const FicQtPlanes& P)
{
    if (hipMemsetAsync(top_sum, 0, (size_t)P.planes * sizeof(unsigned long long), s) != hipSuccess) return -1;
    const FicQtLevels L = qt_levels_arg(sse, nullptr, nullptr, Rw, nl, B_max, Rw_top, Ntop, 0, P, false);
    hipLaunchKernelGGL(k_qt_rd_keys, dim3((Ntop + n1 + 255) / 256, P.planes), dim3(256), 0, s, L, n1, keys, gains, top_sum);
    FIC_LAUNCH_CHECK();
    return 0;
}

int fic_launch_qt_select_w(const uint32_t* keys, const long long* gains, uint32_t n, const unsigned long long* total,
                           unsigned long long* work, hipStream_t s, const FicQtPlanes& P)
{
    if (hipMemsetAsync(work, 0, (size_t)P.planes * FIC_QT_SELECT_W_WORDS * sizeof(unsigned long long), s) != hipSuccess) return -1;
    if (hipMemsetAsync(P.param, 0, (size_t)P.planes * sizeof(uint32_t), s) != hipSuccess) return -1;      // k_qt_select_final_w's atomicMax
    const uint32_t need = (n + 255u) / 256u, nb = need < 1024u ? (need ? need : 1u) : 1024u;      // beyond: the grid stride
    for (int pass = 0; pass < 4; pass++) {
        hipLaunchKernelGGL(k_qt_select_hist_w, dim3(nb, P.planes), dim3(256), 0, s, keys, gains, n, total, P.values, (long long*)work, pass);
        FIC_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_qt_select_final_w, dim3(nb, P.planes), dim3(256), 0, s, keys, gains, n, total, P.values, work, P.param);
    FIC_LAUNCH_CHECK();
    return 0;
}

template <typename Fmt>
int fic_launch_decode_paint_leaves(const typename Fmt::Px* scaled, typename Fmt::Px* image, const typename Fmt::Leaf* lv, int n,
                                   FicDecodeState* state, uint32_t* sqbuf, int counter, const FicGeom& g, hipStream_t s)
{
    if (n <= 0) return 0;
    auto k = g.B == 4 ? k_decode_paint_leaves<Fmt, 4> : (g.B == 8 ? k_decode_paint_leaves<Fmt, 8> : (g.B == 16 ? k_decode_paint_leaves<Fmt, 16> :
             (g.B == 32 ? k_decode_paint_leaves<Fmt, 32> : k_decode_paint_leaves<Fmt, 64>)));      // 32, 64: zoomed decodes only
    const int segs = g.B <= 16 ? 1 : g.B / (sizeof(typename Fmt::Px) == 1 ? 16 : 4);               // qt_paint_seg
    hipLaunchKernelGGL(k, dim3((n * g.B * segs + 255) / 256), dim3(256), 0, s, scaled, image, lv, n, state, sqbuf, counter, g);
    FIC_LAUNCH_CHECK();
    return 0;
}

template <typename Fmt>
int fic_launch_qt_resolve(const int32_t* leaves, const int* n_leaves, const FicQtDecode& D, int planes, int32_t* entries, int32_t* cells,
                          int32_t* cover, FicDecodeState* state, hipStream_t s)
{
    if (hipMemsetAsync(cells, 0xFF, (size_t)planes * D.Nr_min * sizeof(int32_t), s) != hipSuccess) return -1;      // every cell -1
    if (hipMemsetAsync(cover, 0, (size_t)planes * sizeof(int32_t), s) != hipSuccess) return -1;
    hipLaunchKernelGGL(k_qt_resolve<Fmt>, dim3((D.Nr_min + 255) / 256, planes), dim3(256), 0, s, leaves, n_leaves, D, entries, cells, cover, state);
    FIC_LAUNCH_CHECK();
    return 0;
}

template <typename Fmt, int S>
static int qt_paint_planes(const typename Fmt::Px* scaled, typename Fmt::Px* image, const int32_t* entries, const int32_t* cells,
                           const int32_t* cover, FicDecodeState* state, uint32_t* sqbuf, int counter, bool collage, const FicQtDecode& D,
                           int planes, hipStream_t s)
{
    const FicGeom& g = D.g[0];
    const FicQtPaint A{g.W, g.H, D.zoom * D.B_min, D.Rw_min, D.Nr_min, D.zoom * D.B_max, {D.g[0].Dw, D.g[1].Dw, D.g[2].Dw}};
    auto k = collage ? k_qt_paint_planes<Fmt, S, true> : k_qt_paint_planes<Fmt, S, false>;
    const int threads = g.W / S * g.H;
    hipLaunchKernelGGL(k, dim3((threads + 255) / 256, planes), dim3(256), 0, s, scaled, image, entries, cells, cover, state, sqbuf, counter, A);
    FIC_LAUNCH_CHECK();
    return 0;
}

template <typename Fmt>
int fic_launch_qt_paint_planes(const typename Fmt::Px* scaled, typename Fmt::Px* image, const int32_t* entries, const int32_t* cells,
                               const int32_t* cover, FicDecodeState* state, uint32_t* sqbuf, int counter, bool collage, const FicQtDecode& D,
                               int planes, hipStream_t s)
{
    const int cs = D.zoom * D.B_min;                       // a segment stays inside a cell: 4 ARGB pixels, min(16, cs) grey ones
    if constexpr (sizeof(typename Fmt::Px) == 4)
        return qt_paint_planes<Fmt, 4>(scaled, image, entries, cells, cover, state, sqbuf, counter, collage, D, planes, s);
    else if (cs == 4)
        return qt_paint_planes<Fmt, 4>(scaled, image, entries, cells, cover, state, sqbuf, counter, collage, D, planes, s);
    else if (cs == 8)
        return qt_paint_planes<Fmt, 8>(scaled, image, entries, cells, cover, state, sqbuf, counter, collage, D, planes, s);
    else
        return qt_paint_planes<Fmt, 16>(scaled, image, entries, cells, cover, state, sqbuf, counter, collage, D, planes, s);
}

// the batched handle's two formats
#define FIC_QT_INSTANTIATE_DECODE(Fmt)                                                                                                \
    template int fic_launch_qt_resolve<Fmt>(const int32_t*, const int*, const FicQtDecode&, int, int32_t*, int32_t*, int32_t*,        \
                                            FicDecodeState*, hipStream_t);                                                            \
    template int fic_launch_qt_paint_planes<Fmt>(const Fmt::Px*, Fmt::Px*, const int32_t*, const int32_t*, const int32_t*,            \
                                                 FicDecodeState*, uint32_t*, int, bool, const FicQtDecode&, int, hipStream_t);
FIC_QT_INSTANTIATE_DECODE(QtGrey)
FIC_QT_INSTANTIATE_DECODE(QtRgbIso)

#define FIC_QT_INSTANTIATE(Fmt)                                                                                                      \
    template int fic_launch_leaf_sse<Fmt>(const Fmt::Px*, const Fmt::Px*, const int32_t*, const int32_t*, uint32_t*, const FicGeom&,  \
                                          hipStream_t, const FicQtPlanes&);                                                           \
    template int fic_launch_qt_compact<Fmt>(const uint32_t* const*, const int32_t* const*, const int32_t* const*, const int*, int,    \
                                            int, int, int, int*, int*, int32_t*, hipStream_t, const FicQtPlanes&);                    \
    template int fic_launch_qt_compact_rd<Fmt>(const uint32_t* const*, const int32_t* const*, const int32_t* const*, const int*, int, \
                                               int, int, int, const uint32_t*, const uint32_t*, int*, int*, int32_t*, hipStream_t,    \
                                               const FicQtPlanes&);                                                                   \
    template int fic_launch_decode_paint_leaves<Fmt>(const Fmt::Px*, Fmt::Px*, const Fmt::Leaf*, int, FicDecodeState*, uint32_t*,     \
                                                     int, const FicGeom&, hipStream_t);
FIC_QT_INSTANTIATE(QtGrey)
FIC_QT_INSTANTIATE(QtRgb)
FIC_QT_INSTANTIATE(QtRgbIso)
