/*
 * fic.h -- C ABI of libfic_hip.so: the MI355X (gfx950) drop-in for the grey encode hot path
 * of bvk_ss19.FractalCompression (LariWa/Fractal-Image-Compression).
 *
 * The reference has no FFI seam of its own; the boundary is the body of
 * FractalCompression.encodeGrayScale between pool build and writeData
 * (src/bvk_ss19/FractalCompression.java:119-159), reached through
 * FractalCompression.encode(RasterImage, DataOutputStream) (FractalCompression.java:54).
 * Each entry point below names the reference code it replaces.  Plain pointers and sizes
 * only; INTEGRATION.md shows the JNI stub that binds them under the reference's own
 * Java entry point.
 *
 * Conventions
 *   - every int-returning function returns FIC_OK (0) or a negative FIC_E_* code;
 *     fic_last_error() then holds a human-readable message for the calling thread.
 *     The reference throws unchecked exceptions on bad geometry; the JNI
 *     shim turns a negative code into a thrown java.lang.Exception.
 *   - the library never retains caller pointers past return.
 *   - B = FractalCompression.blockgroesse (FractalCompression.java:14), wK =
 *     FractalCompression.widthKernel (:15).  Supported: B in {4, 8, 16} (the GUI's slider
 *     values, RLEAppController.java:131), 1 <= wK <= min(Dw, Dh); wK == Dw == Dh is full search.
 *   - n_iso = 1 is the reference algorithm (bit-identical); n_iso = 8 is this build's
 *     extension (the 8 isometries of the square; order documented in DESIGN.md).
 *   - there is NO CPU fallback: without a usable HIP device every compute entry fails
 *     with FIC_E_NO_DEVICE.
 */
#ifndef FIC_H
#define FIC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FIC_API __attribute__((visibility("default")))

#define FIC_OK 0
#define FIC_E_GEOMETRY (-1)    /* W,H,B combination the reference cannot encode (AIOOBE / div-by-zero there) */
#define FIC_E_WINDOW (-2)      /* wK outside 1..min(Dw,Dh)  (negative index in FractalCompression.java:145) */
#define FIC_E_ARGUMENT (-3)    /* null pointer, bad n_iso, bad plane/range span ... */
#define FIC_E_NO_DEVICE (-4)   /* no HIP device / device index out of range */
#define FIC_E_HIP (-5)         /* a HIP runtime call failed (message has the hipError string) */
#define FIC_E_NOT_GREY (-6)    /* argb input has r!=g or g!=b somewhere (isGreyScale, FractalCompression.java:32-45) */
#define FIC_E_STATE (-7)       /* call order: no input set / nothing encoded yet */
#define FIC_E_CAPACITY (-8)    /* output buffer too small */

typedef struct fic_ctx fic_ctx;

/* ---- library / device ------------------------------------------------------------------ */
FIC_API const char* fic_version(void);
FIC_API const char* fic_last_error(void);
FIC_API int fic_last_error_code(void);   /* code of the last failure on this thread (for NULL returns) */
FIC_API int fic_device_count(void);

/* Block-grid geometry exactly as encodeGrayScale derives it (FractalCompression.java:111-116)
 * and createCodebuch sizes the pool (:1019-1022).  Also the validator: FIC_E_GEOMETRY for
 * sizes on which the reference throws.  Any out pointer may be NULL. */
FIC_API int fic_geometry(int w, int h, int B, int* Rw, int* Rh, int* Dw, int* Dh);

/* isGreyScale (FractalCompression.java:32-45) on a host ARGB buffer: 1 grey, 0 colour. */
FIC_API int fic_is_greyscale_argb(const int32_t* argb, int w, int h);

/* ---- one-shot host-buffer encode (what the JNI shim binds) ------------------------------ */
/* Replaces the search of encodeGrayScale (FractalCompression.java:119-159): pool build
 * (createCodebuch :1015-1050), per-range window selection (:128-150), getBestDomainblock
 * (:613-644) with getErrorVarianceCovariance (:655-687).
 *   argb      RasterImage.argb, w*h ints, only (argb>>16)&0xff is read (:596, :977)
 *   idx_local [N_r] imageInfo[j][0] -- window-local candidate index
 *   a, b      [N_r] imageInfo[j][1..2] -- unquantised float32, bit-exact (needed by
 *             getBestGeneratedCollage :287); a NaN is returned as 0x7FC00000
 *   iso       [N_r] winning isometry id, all 0 for n_iso = 1; may be NULL
 *   qrows     [N_r][3] the ints writeData emits per range (:242-244); may be NULL
 * device: HIP device ordinal. */
FIC_API int fic_encode_gray_argb(const int32_t* argb, int w, int h, int B, int wK, int n_iso, int device,
                                 int32_t* idx_local, float* a, float* b, int32_t* iso, int32_t* qrows);
/* Same with the R channel already extracted (one byte per pixel, scanline order). */
FIC_API int fic_encode_gray_u8(const uint8_t* gray, int w, int h, int B, int wK, int n_iso, int device,
                               int32_t* idx_local, float* a, float* b, int32_t* iso, int32_t* qrows);

/* The same call sharded over the first n_gpus HIP devices of the node, still ONE synchronous call on one host thread --
 * what FractalCompression.encode (FractalCompression.java:54-59) is to its caller (RLEAppController.java:172-188).  The
 * range loop it replaces (:125-159) carries no state between iterations: device g sweeps a contiguous, tile-aligned span
 * of range blocks against its own replica of the pool (built from the replicated image), and the 24-byte codebook
 * records are gathered to device 0 with one grouped RCCL send/recv over xGMI (librccl is loaded on first use; n_gpus = 1
 * is exactly fic_encode_gray_argb on device 0 and needs no RCCL).  Results do not depend on n_gpus.
 * Environment: FIC_GATHER=copy replaces the RCCL gather by peer-to-peer copies; FIC_FAKE_DEVICES=k (test knob) lets
 * n_gpus exceed the visible devices up to k, logical devices sharing the real ones round-robin (gather by device copies:
 * RCCL does not allow two ranks on one device). */
FIC_API int fic_encode_gray_argb_multi(const int32_t* argb, int w, int h, int B, int wK, int n_iso, int n_gpus,
                                       int32_t* idx_local, float* a, float* b, int32_t* iso, int32_t* qrows);
FIC_API int fic_encode_gray_u8_multi(const uint8_t* gray, int w, int h, int B, int wK, int n_iso, int n_gpus,
                                     int32_t* idx_local, float* a, float* b, int32_t* iso, int32_t* qrows);

/* The one-shot entries (grey and RGB) keep the device working sets of the last few geometries (the GUI
 * re-encodes the same image on every slider move, RLEAppController.java:125-145); this frees them, and the RCCL communicators of the multi-device entries. */
FIC_API void fic_release_cache(void);

/* writeData, grey branch (FractalCompression.java:230-246): big-endian int32 header
 * {0, w, h, B, wK} then qrows.  Returns bytes written (20 + 12*n_ranges) or a negative code. */
FIC_API int64_t fic_write_run_gray(const int32_t* qrows, int n_ranges, int w, int h, int B, int wK, uint8_t* out,
                                   int64_t capacity);

/* ---- handle API: device-resident, batched planes, range shards --------------------------- */
/* A context owns the working set for `planes` grey images of one geometry on one device
 * (config 5: 192 planes of 1024x1024; multi-GPU: one context per rank). */
FIC_API fic_ctx* fic_ctx_create(int device, int w, int h, int B, int wK, int n_iso, int planes);
FIC_API void fic_ctx_destroy(fic_ctx* ctx);

/* Input: host bytes [planes][h][w] (copied), host ARGB (copied + R extracted on device), or a
 * device pointer to bytes [planes][h][w] that stays owned by the caller and must remain valid
 * until fic_ctx_sync (no copy; this is the path bench.py times: inputs resident in HBM).
 * The device pointer is read by every later fic_ctx_encode, at encode time and on that encode's
 * stream, not when it is set: what the caller writes there in stream order before an encode is
 * what gets encoded.  Its address must be a multiple of 8 (the widest load of the caller's bytes;
 * plane offsets p*w*h and row offsets keep that alignment for every accepted geometry); any other
 * address is refused with FIC_E_ARGUMENT and the input in force stays.  A later
 * fic_ctx_set_gray_host / fic_ctx_set_argb_host switches back to the context's own copy and never
 * writes through the device pointer. */
FIC_API int fic_ctx_set_gray_host(fic_ctx* ctx, const uint8_t* gray);
FIC_API int fic_ctx_set_argb_host(fic_ctx* ctx, const int32_t* argb);
FIC_API int fic_ctx_set_gray_device(fic_ctx* ctx, const void* dev_gray);

/* Asynchronous encode of range blocks [range_begin, range_begin+range_count) of every plane on
 * `hip_stream` (a hipStream_t, NULL = default stream): pool build + range prep + sweep +
 * finalise.  range_count < 0 means "to the end".  Multi-GPU sharding calls this
 * with a different span per rank; results for other ranges are left untouched.
 * Streams: a context's scratch and result arrays are shared by all its encodes.  Encodes issued
 * on one stream are ordered by it.  An encode issued on ANOTHER stream than the context's last
 * one starts only after that earlier encode has finished (the call waits for it on the host), so
 * the last call wins whatever the streams (after fic_ctx_sync nothing is pending, and the next
 * encode waits for nothing: the old stream may be destroyed by then); fic_ctx_sync, the host getters, collage, decode and
 * the set_*_host entries wait on the stream of the last encode.  The result and record device
 * pointers below never change over the life of the context. */
FIC_API int fic_ctx_encode(fic_ctx* ctx, int range_begin, int range_count, void* hip_stream);
FIC_API int fic_ctx_sync(fic_ctx* ctx);

/* Results.  Host copies are [planes][N_r] ([planes][N_r][3] for qrows); any pointer may be NULL. */
FIC_API int fic_ctx_get_results_host(fic_ctx* ctx, int32_t* idx_local, float* a, float* b, int32_t* iso,
                                     int32_t* qrows, int32_t* idx_global, float* err);
/* Device pointers of the same arrays (for an RCCL gather by the host layer). */
FIC_API int fic_ctx_result_device_ptrs(fic_ctx* ctx, void** idx_local, void** a, void** b, void** iso, void** qrows,
                                       void** idx_global, void** err);

/* The same rows packed as the unit of the multi-GPU codebook gather: device pointer to int32
 * [planes][N_r][6] = {idx_local, a bits, b bits, iso, (int)(a*100), (int)b} (imageInfo[j] of
 * FractalCompression.java:156 + the ints writeData emits, :242-244), written by every fic_ctx_encode for the range
 * span it covered.  Owned by the context. */
FIC_API int fic_ctx_records_device_ptr(fic_ctx* ctx, void** records);

/* getBestGeneratedCollage (FractalCompression.java:269-300): grey ARGB [planes][h][w] of the
 * one-step collage from the unquantised a,b of the last encode (all ranges must be encoded). */
FIC_API int fic_ctx_collage_host(fic_ctx* ctx, int32_t* argb_out);

/* ---- joint-RGB encode ------------------------------------------------------------------------- */
/* encodeRGB (FractalCompression.java:171-219), what FractalCompression.encode dispatches to for
 * colour input (:55-58): scaleImageRGB (:901-962), createCodebuchRGB (:1058-1093) + Domainblock RGB
 * ctor (Domainblock.java:30-41), getBestDomainblockRGB (:697-735), getErrorVarianceCovarianceRGB
 * (:760-808).  One contrast `a` for the three channels, three brightness values.
 *   idx_local, a, bR, bG, bB  [N_r] = imageInfoRGB[j][0..4], unquantised float32 (NaN as 0x7FC00000)
 *   qrows5        [N_r][5] the ints writeData emits (:250-254); may be NULL
 *   collage_argb  getBestGeneratedCollageRGB (:308-347), w*h ARGB ints; may be NULL */
FIC_API int fic_encode_rgb_argb(const int32_t* argb, int w, int h, int B, int wK, int device, int32_t* idx_local,
                                float* a, float* bR, float* bG, float* bB, int32_t* qrows5, int32_t* collage_argb);
/* Handle API of the same path: the device-resident working set of `planes` colour images of one geometry (a batch of
 * config-5 style images, or one image encoded again and again); same kernels, same bits as fic_encode_rgb_argb per image.
 * Input: host ARGB [planes][h][w] (copied) or a device pointer that stays owned by the caller until fic_rgb_ctx_sync.  As
 * for fic_ctx_set_gray_device the device pointer is read at encode time, on the encode's stream; its address must be a
 * multiple of 4 (every kernel loads the pixels as int32), else FIC_E_ARGUMENT and the input in force stays.
 * fic_rgb_ctx_encode is asynchronous on hip_stream; with_collage != 0 also builds getBestGeneratedCollageRGB (:308-347).
 * Streams, as for fic_ctx_encode: an encode issued on another stream than the context's last one starts only after that
 * earlier encode has finished (the call waits for it on the host); getters, decode and fic_rgb_ctx_sync wait on the last stream.
 * Results: [planes][N_r] arrays ([planes][N_r][5] qrows5, [planes][h][w] collage); any pointer may be NULL.
 * fic_rgb_ctx_decode_host runs decodeRGB (:430-508) from the context's quantised rows: argb_out [planes][h][w],
 * avg_error_out / iterations_out [planes] (may be NULL). */
typedef struct fic_rgb_ctx fic_rgb_ctx;
FIC_API fic_rgb_ctx* fic_rgb_ctx_create(int device, int w, int h, int B, int wK, int planes);
FIC_API void fic_rgb_ctx_destroy(fic_rgb_ctx* ctx);
FIC_API int fic_rgb_ctx_set_argb_host(fic_rgb_ctx* ctx, const int32_t* argb);
FIC_API int fic_rgb_ctx_set_argb_device(fic_rgb_ctx* ctx, const void* dev_argb);
FIC_API int fic_rgb_ctx_encode(fic_rgb_ctx* ctx, int with_collage, void* hip_stream);
FIC_API int fic_rgb_ctx_sync(fic_rgb_ctx* ctx);
/* "sweep": 0 (default) = automatic, 1 = the VALU sweeps, 2 = the matrix-core full search (k_sweep_q<NK, 3>: prune on the
 * MFMA output, flagged pairs with the reference's sequential f32 sums; full search only).  All choices give the same
 * bits.  The environment variable FIC_RGB_SWEEP=1|2 overrides.  fic_rgb_ctx_last_sweep: what the last encode ran (1 / 2).
 * "chunks": pool chunks of the matrix-core sweep (0 = automatic; results do not depend on it). */
FIC_API int fic_rgb_ctx_set_option(fic_rgb_ctx* ctx, const char* name, int value);
FIC_API int fic_rgb_ctx_last_sweep(fic_rgb_ctx* ctx);
/* Test hooks of the matrix-core RGB sweep, with the contracts of fic_ctx_last_kernel and fic_ctx_sweep_stats: the name of the
 * sweep kernel the last encode launched -- "k_sweep_q<4, 3, false>" (one pool chunk), "k_sweep_q<4, 3, true>" (several) or
 * "k_sweep_qs<4, 3>" (several short ones) for "sweep" = 2, the VALU kernel's name for "sweep" = 1 -- and, after
 * fic_rgb_ctx_set_option(ctx, "sweep_stats", 1), the same eight counters summed over the planes encoded since the last
 * reset.  Neither changes what is computed. */
FIC_API int fic_rgb_ctx_last_kernel(fic_rgb_ctx* ctx, char* out, int capacity);
FIC_API int fic_rgb_ctx_sweep_stats(fic_rgb_ctx* ctx, uint64_t* out8, int reset);
FIC_API int fic_rgb_ctx_get_results_host(fic_rgb_ctx* ctx, int32_t* idx_local, float* a, float* bR, float* bG, float* bB,
                                         int32_t* qrows5, int32_t* collage_argb);
FIC_API int fic_rgb_ctx_decode_host(fic_rgb_ctx* ctx, int32_t* argb_out, float* avg_error_out, int* iterations_out);
/* Joint RGB with the 8 isometries of the square (n_iso = 8; an extension like the grey one: the reference has none).  The
 * error of getErrorVarianceCovarianceRGB is applied to the explicitly permuted domain block D_k[i] = D[src_k(i)], src_k the
 * map of the grey extension (k = 0 identity, 1 rot90cw, 2 rot180, 3 rot270cw, 4 mirror L-R, 5 mirror T-B, 6 transpose,
 * 7 anti-transpose): kovarianz_k = sum_i greyR[i] * greyD[src_k(i)] accumulated in f32 in the range block's order
 * i = 0..n-1; varianzRange, varianzDomain, varianzSquare and the channel means are those of the unpermuted block.  Scan:
 * candidates in window order and k = 0..7 inside a candidate, strict '<' (a tie goes to the lower (c, k)).  The collage and
 * the decoder paint pixel (rx, ry) of a range block from the domain pixel at src_k(rx, ry).
 *   n_iso   1 or 8 (FIC_E_ARGUMENT otherwise, before any device work); 1 gives the bits of the entries above
 *   iso     [N_r] winning isometry (all 0 with n_iso = 1); may be NULL.  qrows5 keeps its shape: the .run format has no
 *           isometry column, so an n_iso = 8 codebook is written with fic_write_run_rgb_iso (tag 5, below) and decoded with
 *           fic_decode_rgb_iso_run, or from its context (fic_rgb_ctx_decode_host / fic_rgb_ctx_decode_zoom_host)
 * Sweep policy: that of fic_rgb_ctx_encode with the pair count times 8 -- the matrix-core sweep ("k_sweep_q<NK, 4, ..>" /
 * "k_sweep_qs<NK, 4>": 8 permuted range columns per block, flagged pairs evaluated exactly in the range block's order) for full
 * search when 8 N_r N_d >= 3e7 or B = 16, else the VALU sweeps ("k_sweep_rgb_fast_iso<n>": full search at B = 4 / 8,
 * "k_sweep_rgb_iso": windowed search); "sweep", FIC_RGB_SWEEP, "chunks", "q_eshift" and "sweep_stats" work as with n_iso = 1, all
 * choices give the same bits.  A window of 2^28 or more candidates is FIC_E_GEOMETRY (the search key carries c * 8 + k). */
FIC_API int fic_encode_rgb_iso_argb(const int32_t* argb, int w, int h, int B, int wK, int n_iso, int device, int32_t* idx_local,
                                    float* a, float* bR, float* bG, float* bB, int32_t* iso, int32_t* qrows5,
                                    int32_t* collage_argb);
FIC_API fic_rgb_ctx* fic_rgb_ctx_create_iso(int device, int w, int h, int B, int wK, int n_iso, int planes);
/* iso [planes][N_r] of the last encode (zeros on an n_iso = 1 context) */
FIC_API int fic_rgb_ctx_get_iso_host(fic_rgb_ctx* ctx, int32_t* iso);

/* writeData, RGB branch (FractalCompression.java:230-238, 248-257): header {1,w,h,B,wK} + 5 ints per row. */
FIC_API int64_t fic_write_run_rgb(const int32_t* qrows5, int n_ranges, int w, int h, int B, int wK, uint8_t* out,
                                  int64_t capacity);

/* ---- decoder --------------------------------------------------------------------------------- */
/* FractalCompression.decode on a complete grey .run stream (FractalCompression.java:547-553 ->
 * decodeGreyScale :356-421): header, rows, calculateIndices (:853-893), then up to 50 iterations
 * of {rebuild pool from the current image, repaint every range block, accumulate the squared
 * change}, stopping when the mean change drops below 1 (:413-415).
 *   gray_out        R channel of the decoded image, w*h bytes (the reference returns grey ARGB)
 *   avg_error_io    in: FractalCompression.avgError before the call (the static is never reset,
 *                   :20,:407); out: its value after the call = the GUI's "MSE" label
 *                   (RLEAppController.java:180).  May be NULL (treated as 0).
 *   iterations      iterations executed; may be NULL.
 * avgError is Java's float accumulation (:407), one add per pixel in range-block order: taken from the exact integer sum
 * when every partial sum is an exact float, re-accumulated sequentially in that order otherwise (large or
 * non-converging decodes), so the returned value and the "< 1" decision (:413-415) match for any size. */
FIC_API int fic_decode_gray_run(const uint8_t* run, int64_t len, int device, uint8_t* gray_out, int64_t capacity,
                                int* w, int* h, float* avg_error_io, int* iterations);
/* decodeRGB (FractalCompression.java:430-508) on a complete colour .run stream (isRGB != 0):
 * rows {idx, a*1e6, bR*1e5, bG*1e5, bB} (:446-450), scaleImageRGB pool, per-channel repaint, the
 * three squared channel changes summed per pixel (:493).  argb_out: w*h ARGB ints. */
FIC_API int fic_decode_rgb_run(const uint8_t* run, int64_t len, int device, int32_t* argb_out,
                               int64_t capacity_pixels, int* w, int* h, float* avg_error_io, int* iterations);
/* The same loop driven from the context's last encode: quantised rows (and isometry ids, so
 * n_iso = 8 codebooks decode too) stay on the device.  gray_out [planes][h][w]; avg_error_out and
 * iterations_out [planes], may be NULL.  Every range block must have been encoded. */
FIC_API int fic_ctx_decode_host(fic_ctx* ctx, uint8_t* gray_out, float* avg_error_out, int* iterations_out);

/* ---- decoding at 2x or 4x zoom ------------------------------------------------------------------ */
/* A codebook row says "paint this range block from that domain block with contrast a and brightness b"; nothing in it
 * depends on the pixel size.  The geometry is scale-free (Rw = w / B, Dw = 2 Rw - 3, domain stride B / 4), so the stream of
 * a w x h, block-B image is also a stream of a zoom*w x zoom*h image with block zoom*B.  Each entry below is its unzoomed
 * twin with `int zoom` in {1, 2, 4} (FIC_E_ARGUMENT otherwise) and runs exactly the twin's loop on the geometry
 * (zoom*w, zoom*h, zoom*B, wK): the same start image, the rows unchanged, scaleImage / scaleImageRGB of the current zoomed
 * image (the `x + 1 >= height` quirk evaluated at the zoomed size), domain origin (c * zoom*B / 4, r * zoom*B / 4), the same
 * per-pixel arithmetic, isometries of side zoom*B, avgError summed in Java's float order over the zoomed pixels (range block by
 * range block, pixel rows within a block) and divided by (float) (zoom*w * zoom*h), at most 50 iterations, stop at < 1.  A
 * quadtree leaf {x, y, B} becomes {zoom*x, zoom*y, zoom*B} in its stream order with its own level's window.  zoom = 1 is the
 * twin bit for bit.  The stream itself must be one the twin accepts (its own B in {4, 8, 16}: the sides 32 and 64 exist for
 * zoomed decodes only); *w / *h return the zoomed size and the output needs zoom^2 * w * h pixels (FIC_E_CAPACITY);
 * FIC_E_GEOMETRY when the zoomed image exceeds the 32-bit limits of the geometry.  All checks happen before any device work. */
FIC_API int fic_decode_gray_run_zoom(const uint8_t* run, int64_t len, int zoom, int device, uint8_t* gray_out, int64_t capacity,
                                     int* w, int* h, float* avg_error_io, int* iterations);
FIC_API int fic_decode_rgb_run_zoom(const uint8_t* run, int64_t len, int zoom, int device, int32_t* argb_out,
                                    int64_t capacity_pixels, int* w, int* h, float* avg_error_io, int* iterations);
FIC_API int fic_decode_quadtree_run_zoom(const uint8_t* run, int64_t len, int zoom, int device, uint8_t* gray_out, int64_t capacity,
                                         int* w, int* h, float* avg_error_io, int* iterations);
FIC_API int fic_decode_rgb_quadtree_run_zoom(const uint8_t* run, int64_t len, int zoom, int device, int32_t* argb_out,
                                             int64_t capacity_pixels, int* w, int* h, float* avg_error_io, int* iterations);
/* fic_ctx_decode_host at zoom: gray_out [planes][zoom*h][zoom*w].  Zooms a fixed-B n_iso = 8 codebook straight from its
 * context (as a stream it goes through fic_write_run_gray_iso / fic_decode_gray_iso_run, tag 4, below), and batched planes. */
FIC_API int fic_ctx_decode_zoom_host(fic_ctx* ctx, int zoom, uint8_t* gray_out, float* avg_error_out, int* iterations_out);
/* The colour twin: fic_rgb_ctx_decode_host at zoom, argb_out [planes][zoom*h][zoom*w], for n_iso = 1 and n_iso = 8 contexts.
 * zoom = 1 gives the bits of fic_rgb_ctx_decode_host. */
FIC_API int fic_rgb_ctx_decode_zoom_host(fic_rgb_ctx* ctx, int zoom, int32_t* argb_out, float* avg_error_out, int* iterations_out);

/* ---- fixed-B streams with an isometry column (tags 4 and 5) -------------------------------------- */
/* An extension like the quadtree streams: the .run format of the reference has no place for the isometry of an n_iso = 8
 * codebook.  Big-endian int32 like writeData: header {4, w, h, 0, B, wK} (grey) or {5, w, h, 0, B, wK} (colour), then per range
 * block in scanline order {idx_local, qa, qb, iso} or {idx_local, q1, q2, q3, q4, iso}; iso in 0..7 with the numbering of
 * fic_encode_rgb_iso_argb.  An n_iso = 1 codebook is written with a column of zeros.  The 0 sits where a .run holds its block
 * size: Java's decodeRGB divides by it, fic_decode_rgb_run refuses it with FIC_E_GEOMETRY, fic_decode_gray_run refuses the
 * non-zero tag with FIC_E_NOT_GREY and the quadtree readers refuse any tag but their own, so no older reader misreads the stream.
 * Writers, host only: return the bytes written (24 + 4 * (QW + 1) * N_r) or a negative code -- FIC_E_ARGUMENT for a null
 * pointer, n_ranges other than the geometry's N_r or an iso outside 0..7, FIC_E_GEOMETRY / FIC_E_WINDOW as fic_geometry and the
 * window check give them, FIC_E_CAPACITY for a short buffer. */
FIC_API int64_t fic_write_run_gray_iso(const int32_t* qrows, const int32_t* iso, int n_ranges, int w, int h, int B, int wK,
                                       uint8_t* out, int64_t capacity);
FIC_API int64_t fic_write_run_rgb_iso(const int32_t* qrows5, const int32_t* iso, int n_ranges, int w, int h, int B, int wK,
                                      uint8_t* out, int64_t capacity);
/* Decoders, with `zoom` in {1, 2, 4} as in the section above: the loop of fic_decode_gray_run_zoom / fic_decode_rgb_run_zoom on
 * the geometry (zoom*w, zoom*h, zoom*B, wK) with range pixel (rx, ry) painted from the domain pixel at src_k(rx, ry) of side
 * zoom*B -- what fic_ctx_decode_zoom_host / fic_rgb_ctx_decode_zoom_host compute on a context that holds the same rows and
 * isometries (pixels, avgError, iterations); with a column of zeros, what the tag-0 / tag-1 stream of the same rows decodes
 * to.  avg_error_io as in fic_decode_gray_run; *w / *h return the zoomed size (also on FIC_E_CAPACITY).  Checked on the host
 * before any device work: FIC_E_ARGUMENT for another tag, a non-zero 4th int, a length other than the header's (truncated or
 * oversized), an idx_local outside 0 .. wK^2 - 1, an iso outside 0..7 or a zoom outside {1, 2, 4}; FIC_E_GEOMETRY /
 * FIC_E_WINDOW for a header the geometry or window check refuses. */
FIC_API int fic_decode_gray_iso_run(const uint8_t* run, int64_t len, int zoom, int device, uint8_t* gray_out, int64_t capacity,
                                    int* w, int* h, float* avg_error_io, int* iterations);
FIC_API int fic_decode_rgb_iso_run(const uint8_t* run, int64_t len, int zoom, int device, int32_t* argb_out,
                                   int64_t capacity_pixels, int* w, int* h, float* avg_error_io, int* iterations);

/* ---- quadtree (variable block size) grey codec -------------------------------------------------- */
/* An extension like n_iso = 8: the reference encodes with one block size (FC:14).  Levels B_max in {8, 16}, B_min in {4, 8},
 * B_min < B_max; w and h multiples of B_max.  Every level B = B_max, B_max/2, ..., B_min is encoded exactly as
 * fic_encode_gray_u8(gray, w, h, B, wK_B, n_iso) encodes it, with wK_B = Dw_B (full search; square images) when wK = 0, else
 * wK_B = wK (which must be a valid window at every level).  The collage error of a range block is
 * SSE = sum (orig - value)^2 of its QUANTISED row, value = clamp((int) fl(fl(((float) qa / 100f) * d) + (float) qb)) with d the
 * winner's domain pixel (isometry applied) in the 2:1-scaled original: what the decoder paints.  Top-down from B_max a
 * block is split into four iff B > B_min and (double) SSE > (double) threshold * B * B (threshold: mean squared error per
 * pixel; +inf never splits, a negative value always splits down to B_min; NaN is refused).
 *   leaves   int32 [capacity][7] {x, y, B, idx_local, qa, qb, iso}: top-level blocks in scanline order, inside a block depth
 *            first TL, TR, BL, BR; iso = 0 when n_iso = 1.  *n_leaves = the count (also set on FIC_E_CAPACITY).
 * The first version encodes every level in full: the cost is the sum of the fixed-B encodes. */
FIC_API int fic_encode_gray_quadtree_u8(const uint8_t* gray, int w, int h, int B_max, int B_min, int wK, int n_iso, float threshold,
                                        int device, int32_t* leaves, int64_t capacity, int* n_leaves);
FIC_API int fic_encode_gray_quadtree_argb(const int32_t* argb, int w, int h, int B_max, int B_min, int wK, int n_iso,
                                          float threshold, int device, int32_t* leaves, int64_t capacity, int* n_leaves);
/* Quadtree stream, host only: big-endian int32 header {2, w, h, B_max, B_min, wK, n_iso, n_leaves}, then per leaf
 * {B, idx_local, qa, qb} (+ iso when n_iso = 8); positions follow from the order.  The leaves must tile the image in the order
 * above.  Returns the bytes written or a negative code.  Tag 2 is NEW: the reference's FractalCompression.decode reads any
 * non-zero first int as isRGB (FC:547-553) and would misread this stream as a colour .run; fic_decode_gray_run and
 * fic_decode_rgb_run do not accept it either. */
FIC_API int64_t fic_write_run_quadtree(const int32_t* leaves, int n_leaves, int w, int h, int B_max, int B_min, int wK, int n_iso,
                                       uint8_t* out, int64_t capacity);
/* Decoder of a quadtree stream: the loop of decodeGreyScale (FC:356-421) -- grey 128 start, at most 50 iterations, each one
 * the 2:1 scale of the current image and every leaf painted from its own level's domain block, the squared changes summed
 * in Java's float order over the leaves in stream order (pixel rows within a leaf), stop when avgError < 1.  avg_error_io as
 * in fic_decode_gray_run.  The stream is checked before any device work: FIC_E_ARGUMENT for a tag other than 2, sizes that
 * do not tile the image exactly, a B outside the levels, an idx_local outside the level's window, an isometry outside
 * 0..n_iso-1, and a length other than the header's (truncated or oversized).  With threshold = +inf the stream decodes bit
 * for bit like the fixed-B_max .run (pixels, avgError, iterations). */
FIC_API int fic_decode_quadtree_run(const uint8_t* run, int64_t len, int device, uint8_t* gray_out, int64_t capacity, int* w,
                                    int* h, float* avg_error_io, int* iterations);
/* Test hook: the per-level collage SSE arrays of the quadtree encode, levels B_max .. B_min concatenated, [N_r(B)] each in
 * scanline order. */
FIC_API int fic_debug_quadtree_sse(const uint8_t* gray, int w, int h, int B_max, int B_min, int wK, int n_iso, int device,
                                   uint32_t* sse, int64_t capacity);

/* ---- quadtree (variable block size) joint-RGB codec ---------------------------------------------- */
/* The colour twin of the grey quadtree codec above, built on the joint-RGB path (encodeRGB / decodeRGB, FC:171-219,
 * 430-508).  Levels, geometry, wK and the split rule as for the grey codec; no isometries (the reference's colour path has
 * none).  Every level B is encoded exactly as fic_encode_rgb_argb(argb, w, h, B, wK_B) encodes it (the same cached
 * working sets).  The collage error of a range block is that of its QUANTISED row {idx, q1, q2, q3, q4}, what decodeRGB
 * paints: a = (float) q1 / 1e6f, bR = (float) q2 / 1e5f, bG = (float) q3 / 1e5f, bB = (float) q4 (sic), per channel
 * value_c = clamp((int) fl(fl(a * d_c) + b_c)) with d the winner's domain pixel in scaleImageRGB of the original, and
 * SSE = sum over the pixels and R, G, B of (orig_c - value_c)^2.  Split iff B > B_min and (double) SSE > (double) threshold * B * B:
 * threshold is in the unit of decodeRGB's avgError, the squared error per pixel summed over the three channels.
 *   argb     int32 [h][w] packed ARGB (RasterImage.argb)
 *   leaves   int32 [capacity][8] {x, y, B, idx_local, q1, q2, q3, q4} in the grey codec's order; q1..q4 are the level's
 *            qrows5 row.  *n_leaves = the count (also set on FIC_E_CAPACITY). */
FIC_API int fic_encode_rgb_quadtree_argb(const int32_t* argb, int w, int h, int B_max, int B_min, int wK, float threshold,
                                         int device, int32_t* leaves, int64_t capacity, int* n_leaves);
/* Colour quadtree stream, host only: big-endian int32 header {3, w, h, 0, B_max, B_min, wK, n_leaves}, then per leaf
 * {B, idx_local, q1, q2, q3, q4}.  The leaves must tile the image in quadtree order.  Returns the bytes written or a negative
 * code.  The 0 sits where a fixed-B .run holds its block size (FC:234-238): Java's decodeRGB divides by it, fic_decode_rgb_run
 * refuses it with FIC_E_GEOMETRY, fic_decode_gray_run refuses the non-zero tag with FIC_E_NOT_GREY and fic_decode_quadtree_run
 * refuses any tag but 2, so no existing reader misreads the stream. */
FIC_API int64_t fic_write_run_rgb_quadtree(const int32_t* leaves, int n_leaves, int w, int h, int B_max, int B_min, int wK,
                                           uint8_t* out, int64_t capacity);
/* Decoder of a colour quadtree stream: the loop of decodeRGB (FC:430-508) -- generateGrayImage start (0xff808080), at most 50
 * iterations, each one scaleImageRGB of the current image and every leaf painted from its own level's domain block, the
 * per-pixel dR^2 + dG^2 + dB^2 summed in Java's float order over the leaves in stream order (pixel rows within a leaf), stop
 * when avgError < 1.  argb_out int32 [capacity_pixels >= w*h]; avg_error_io as in fic_decode_rgb_run.  The stream is checked
 * before any device work: FIC_E_ARGUMENT for a tag other than 3 or a non-zero 4th int, bad levels or geometry, sizes that do
 * not tile the image, an idx_local outside its level's window, n_leaves outside 1 .. the B_min block count, and a length
 * other than the header's.  With threshold = +inf the stream decodes bit for bit like the fixed-B_max .run that
 * fic_write_run_rgb writes from the same codebook (pixels, avgError, iterations). */
FIC_API int fic_decode_rgb_quadtree_run(const uint8_t* run, int64_t len, int device, int32_t* argb_out, int64_t capacity_pixels,
                                        int* w, int* h, float* avg_error_io, int* iterations);
/* Test hook: the per-level collage SSE arrays of the colour quadtree encode, levels B_max .. B_min concatenated, [N_r(B)]
 * each in scanline order. */
FIC_API int fic_debug_rgb_quadtree_sse(const int32_t* argb, int w, int h, int B_max, int B_min, int wK, int device, uint32_t* sse,
                                       int64_t capacity);

/* ---- quadtree joint-RGB codec with the 8 isometries (tag 6) ------------------------------------- */
/* The colour quadtree codec above with n_iso = 1 or 8 (FIC_E_ARGUMENT otherwise): levels, geometry, wK, split rule, leaf order
 * and argument checks are those of fic_encode_rgb_quadtree_argb; every level B is encoded exactly as
 * fic_encode_rgb_iso_argb(argb, w, h, B, wK_B, n_iso) encodes it (the same cached working sets and sweep policy), and the
 * collage SSE of a range block takes the domain pixel of range pixel (rx, ry) at src_k(rx, ry), k the block's winning
 * isometry: what fic_decode_rgb_quadtree_iso_run paints.
 *   leaves   int32 [capacity][9] {x, y, B, idx_local, q1, q2, q3, q4, iso}.  With n_iso = 1 the first 8 columns are the rows
 *            of fic_encode_rgb_quadtree_argb and iso is 0. */
FIC_API int fic_encode_rgb_quadtree_iso_argb(const int32_t* argb, int w, int h, int B_max, int B_min, int wK, int n_iso,
                                             float threshold, int device, int32_t* leaves, int64_t capacity, int* n_leaves);
/* Stream, host only: header {6, w, h, 0, B_max, B_min, wK, n_leaves}, then per leaf {B, idx_local, q1, q2, q3, q4, iso} in
 * quadtree order (the 0 as in tag 3: no older reader takes the stream).  The rule of fic_write_run_rgb_quadtree, and
 * FIC_E_ARGUMENT for an iso outside 0..7. */
FIC_API int64_t fic_write_run_rgb_quadtree_iso(const int32_t* leaves, int n_leaves, int w, int h, int B_max, int B_min, int wK,
                                               uint8_t* out, int64_t capacity);
/* Decoder with `zoom` in {1, 2, 4}: the loop of fic_decode_rgb_quadtree_run_zoom with every leaf painted through its
 * isometry at side zoom*B.  With a column of zeros it decodes like the tag-3 stream of the same leaves; with threshold = +inf
 * like the tag-5 stream of the fixed-B_max codebook.  Checked before any device work: every check of the tag-3 reader with
 * FIC_E_ARGUMENT (tag other than 6, non-zero 4th int, bad levels, sizes that do not tile, idx_local outside its level's window,
 * n_leaves outside 1 .. the B_min block count, a length other than the header's), an iso outside 0..7 likewise; a geometry or
 * window the levels' own check refuses fails with FIC_E_GEOMETRY / FIC_E_WINDOW. */
FIC_API int fic_decode_rgb_quadtree_iso_run(const uint8_t* run, int64_t len, int zoom, int device, int32_t* argb_out,
                                            int64_t capacity_pixels, int* w, int* h, float* avg_error_io, int* iterations);
/* Test hook with the layout of fic_debug_rgb_quadtree_sse. */
FIC_API int fic_debug_rgb_quadtree_iso_sse(const int32_t* argb, int w, int h, int B_max, int B_min, int wK, int n_iso, int device,
                                           uint32_t* sse, int64_t capacity);

/* ---- quadtree encode to a leaf budget ------------------------------------------- */
/* The quadtree encodes above with a size limit in place of the threshold: the tree of at most max_leaves leaves at the
 * smallest threshold that allows it.  Levels, geometry, wK, per-level codebooks, collage SSE, split rule, leaf order and leaf
 * rows are those of the fixed-threshold entry of the same name; the levels are encoded once, and the threshold is chosen on
 * the device from the SSE arrays of that encode.  With N_top the blocks of side B_max, k(v) = SSE_v * (256 / B^2) for a block v
 * of side B > B_min (v splits under t iff k(v) > 256 t) and e(v) the minimum of k over v and its ancestors, the tree under t has
 * N_top + 3 #{v : e(v) > 256 t} leaves.  Let S = (max_leaves - N_top) / 3 and K the (S+1)-th largest e(v), 0 when there are S
 * or fewer: *threshold_out = the smallest float >= K / 256, which is the smallest non-negative float whose tree has at most
 * max_leaves leaves, and `leaves` is exactly what the fixed-threshold entry returns for it.  Blocks that share the key K all
 * stay whole, so the tree may have fewer than max_leaves leaves; it never has more.
 *   max_leaves     >= N_top, else FIC_E_ARGUMENT (checked with the other arguments, before any device work)
 *   threshold_out  the threshold chosen; set on FIC_E_CAPACITY too, like *n_leaves
 *   stats4         NULL, or uint64 [4] = {collage SSE summed over the leaves, leaves of side B_max, B_max / 2, B_max / 4} */
FIC_API int fic_encode_gray_quadtree_budget_u8(const uint8_t* gray, int w, int h, int B_max, int B_min, int wK, int n_iso,
                                               int64_t max_leaves, int device, int32_t* leaves, int64_t capacity, int* n_leaves,
                                               float* threshold_out, uint64_t* stats4);
FIC_API int fic_encode_gray_quadtree_budget_argb(const int32_t* argb, int w, int h, int B_max, int B_min, int wK, int n_iso,
                                                 int64_t max_leaves, int device, int32_t* leaves, int64_t capacity, int* n_leaves,
                                                 float* threshold_out, uint64_t* stats4);
/* The same for the colour codec (tag 3; threshold in decodeRGB's unit) and for colour with n_iso = 1 or 8 isometries (tag 6). */
FIC_API int fic_encode_rgb_quadtree_budget_argb(const int32_t* argb, int w, int h, int B_max, int B_min, int wK, int64_t max_leaves,
                                                int device, int32_t* leaves, int64_t capacity, int* n_leaves, float* threshold_out,
                                                uint64_t* stats4);
FIC_API int fic_encode_rgb_quadtree_iso_budget_argb(const int32_t* argb, int w, int h, int B_max, int B_min, int wK, int n_iso,
                                                    int64_t max_leaves, int device, int32_t* leaves, int64_t capacity,
                                                    int* n_leaves, float* threshold_out, uint64_t* stats4);
/* Host only: the largest leaf count whose quadtree stream of `tag` (2 grey, 3 colour, 6 colour with isometries) fits
 * max_bytes: a 32-byte header, then 4 (tag 2, n_iso = 1), 5 (tag 2, n_iso = 8), 6 (tag 3) or 7 (tag 6) ints per leaf.  0 when
 * only the header fits.  FIC_E_ARGUMENT for another tag, an n_iso other than 1 or 8, or tag 3 with n_iso = 8; FIC_E_CAPACITY
 * when max_bytes < 32.  Whether the count is a valid budget (>= N_top) is the encode's to say. */
FIC_API int64_t fic_quadtree_leaves_for_bytes(int tag, int n_iso, int64_t max_bytes);
/* Test hook: the budget's radix select alone, on the caller's keys uint32 [n], 1 <= n < 2^31.  *key_out = the key of rank
 * `rank` >= 0 in descending order (rank 0: the largest; 0 for rank >= n), *threshold_out = the smallest float >= key / 256,
 * *above_out = the number of keys greater than the key. */
FIC_API int fic_debug_qt_select(int device, const uint32_t* keys, int64_t n, int64_t rank, uint32_t* key_out, float* threshold_out,
                                int64_t* above_out);

/* ---- quadtree encode by rate-distortion pruning ---------------------------------- */
/* The quadtree encodes above with the tree chosen by what a split buys against what it costs: T(lambda) minimises
 * D + lambda * N over all trees of the ladder, D the collage SSE summed over the leaves and N the number of leaves.  Levels,
 * geometry, wK, per-level codebooks, collage SSE, leaf order and leaf rows are those of the fixed-threshold entry of the same
 * name; the levels are encoded once and lambda is chosen on the device.  Exact integers: with S_v the collage SSE of block v
 * (uint32, the all-ones mark as 2^32 - 1) and an integer 0 <= lambda <= 2^32 - 1,
 *   J(v) = S_v + lambda at side B_min, else min(S_v + lambda, sum of J over the four children);
 *   v wants to split iff that sum is < S_v + lambda (a tie keeps the block whole);
 *   in T(lambda) a block is split iff it and all its ancestors want to.
 * With k(v) the smallest lambda at which v does not want to split, e(v) = min(k(v), k(parent(v))), G_v = S_v - the sum of S over
 * v's children (signed) and N_top the blocks of side B_max: T(lambda) has N(lambda) = N_top + 3 #{v : e(v) > lambda} leaves and
 * the collage SSE D(lambda) = sum S_top - sum_{e(v) > lambda} G_v; N never rises and D never falls as lambda grows, and every
 * T(lambda) has the least collage SSE of all trees with its number of leaves.
 *   search      0: the reference's criterion for the per-level codebooks, 1: least squares
 *   goal/value  FIC_QT_RD_LAMBDA  value = lambda; above 2^32 - 1 is FIC_E_ARGUMENT
 *               FIC_QT_RD_LEAVES  value = max_leaves >= N_top (else FIC_E_ARGUMENT): the smallest lambda whose tree has at most
 *                                 max_leaves leaves, the (S+1)-th largest e(v) with S = (max_leaves - N_top) / 3, 0 when there
 *                                 are S or fewer.  Blocks that share that key all stay whole: the tree may have fewer leaves
 *               FIC_QT_RD_SSE     value = max_sse: the tree of fewest leaves among the T(lambda) with D <= max_sse, and the
 *                                 smallest lambda that gives it (an e(v) or 0).  If even D(0) > max_sse the result is T(0) with
 *                                 *lambda_out = 0 and FIC_OK: the caller sees it in stats4[0] > value
 *   lambda_out  the lambda in force; set on FIC_E_CAPACITY too, like *n_leaves
 *   stats4      NULL, or uint64 [4] as in the budget entries
 * Checked before any device work: null pointers (FIC_E_ARGUMENT), goal outside 0..2, search outside 0..1, the ranges of value
 * above, and the levels, geometry and window as in the fixed-threshold entries.  The leaf tables go through the stream writers
 * and decoders unchanged. */
#define FIC_QT_RD_LAMBDA 0
#define FIC_QT_RD_LEAVES 1
#define FIC_QT_RD_SSE 2
FIC_API int fic_encode_gray_quadtree_rd_u8(const uint8_t* gray, int w, int h, int B_max, int B_min, int wK, int n_iso, int search,
                                           int goal, uint64_t value, int device, int32_t* leaves, int64_t capacity, int* n_leaves,
                                           uint32_t* lambda_out, uint64_t* stats4);
FIC_API int fic_encode_gray_quadtree_rd_argb(const int32_t* argb, int w, int h, int B_max, int B_min, int wK, int n_iso, int search,
                                             int goal, uint64_t value, int device, int32_t* leaves, int64_t capacity, int* n_leaves,
                                             uint32_t* lambda_out, uint64_t* stats4);
/* The same for the colour codec (tag 3 rows, leaves [capacity][8]) and for colour with n_iso = 1 or 8 isometries (tag 6 rows,
 * leaves [capacity][9]). */
FIC_API int fic_encode_rgb_quadtree_rd_argb(const int32_t* argb, int w, int h, int B_max, int B_min, int wK, int search, int goal,
                                            uint64_t value, int device, int32_t* leaves, int64_t capacity, int* n_leaves,
                                            uint32_t* lambda_out, uint64_t* stats4);
FIC_API int fic_encode_rgb_quadtree_iso_rd_argb(const int32_t* argb, int w, int h, int B_max, int B_min, int wK, int n_iso, int search,
                                                int goal, uint64_t value, int device, int32_t* leaves, int64_t capacity,
                                                int* n_leaves, uint32_t* lambda_out, uint64_t* stats4);
/* Test hook: the keys and gains of the pruning alone, no encode.  sse: the levels B_max .. B_min concatenated, as
 * fic_debug_quadtree_sse returns them; keys / gains [N_top (+ the blocks of B_max / 2 with three levels)]: e(v) and G_v, the
 * blocks of B_max in scanline order first, then those of B_max / 2. */
FIC_API int fic_debug_qt_rd_keys(int device, const uint32_t* sse, int w, int h, int B_max, int B_min, uint32_t* keys, int64_t* gains);
/* Test hook: the weighted select of FIC_QT_RD_SSE alone, on the caller's (key, gain) pairs, 1 <= n < 2^31.  With the distinct
 * keys in descending order followed by 0, *key_out = the first boundary at which the sum of gain over the keys > boundary is
 * >= need (0 when none is), *above_out = the number of those keys, *gain_out = their summed gain.  need <= 0 selects the
 * largest key.  Precondition: that sum does not fall from one boundary to the next (the keys and gains of the pruning
 * guarantee it; gains of any sign inside a group of equal keys are fine). */
FIC_API int fic_debug_qt_select_weighted(int device, const uint32_t* keys, const int64_t* gains, int64_t n, int64_t need,
                                         uint32_t* key_out, int64_t* above_out, int64_t* gain_out);

/* ---- batched quadtree encoder handle ------------------------------------------------------------------------- */
/* The quadtree encodes above for `planes` images of one geometry at once, as a handle like fic_ctx / fic_rgb_ctx: the context
 * owns one context per level (created with `planes`) and the device stores of the quadtree layer, reads a caller's device
 * tensor in place and runs asynchronously on the caller's stream.  Plane p of a batch is, bit for bit, what the one-shot entry
 * of the same format returns for image p alone; no new stream format: each plane's table goes through the writers above.
 *   colour   0: grey, leaf rows of 7 ints as fic_encode_gray_quadtree_u8's; 1: joint RGB with the isometry column, rows of 9
 *            ints as fic_encode_rgb_quadtree_iso_argb's, n_iso 1 or 8 (without its last column a row is
 *            fic_encode_rgb_quadtree_argb's)
 * Levels, geometry and window are checked as in the one-shot entries; FIC_E_GEOMETRY also when planes is above 65535 or an
 * index of the context -- planes * (w / B_min) * (h / B_min) * the ints of a row is the largest -- would pass 2^31 - 1.
 * Every check comes before any device work. */
typedef struct fic_qt_ctx fic_qt_ctx;
FIC_API fic_qt_ctx* fic_qt_ctx_create(int device, int colour, int w, int h, int B_max, int B_min, int wK, int n_iso, int planes);
FIC_API void fic_qt_ctx_destroy(fic_qt_ctx* ctx);
/* Input [planes][h][w] under the contract of fic_ctx_set_gray_* / fic_rgb_ctx_set_argb_*: a host image is uploaded once into
 * the context's copy; a device pointer stays the caller's, is handed to every level, never copied and read by every later
 * encode at encode time (address a multiple of 8 for bytes, of 4 for ARGB, else FIC_E_ARGUMENT and the input in force stays).
 * A grey context takes bytes (host or device) or host ARGB; a colour context takes ARGB (host or device). */
FIC_API int fic_qt_ctx_set_gray_host(fic_qt_ctx* ctx, const uint8_t* gray);
FIC_API int fic_qt_ctx_set_argb_host(fic_qt_ctx* ctx, const int32_t* argb);
FIC_API int fic_qt_ctx_set_gray_device(fic_qt_ctx* ctx, const void* dev_gray);
FIC_API int fic_qt_ctx_set_argb_device(fic_qt_ctx* ctx, const void* dev_argb);
/* "search": 0 the reference's criterion for the per-level codebooks, 1 least squares (the `search` of the RD entries). */
FIC_API int fic_qt_ctx_set_option(fic_qt_ctx* ctx, const char* name, int value);
/* The three encodes: one value per plane (host arrays of `planes` values), asynchronous on `hip_stream` under the stream
 * rule of fic_ctx_encode.  The values go up from a pinned buffer of the context and every rule's parameter is read from device
 * memory: the call enqueues everything and returns without waiting for the device.
 *   threshold   the fixed-threshold rule; a NaN is FIC_E_ARGUMENT
 *   budget      the threshold chosen on the device for at most max_leaves[p] leaves (>= N_top, else FIC_E_ARGUMENT); on the
 *               reference's criterion only: FIC_E_ARGUMENT under "search" = 1
 *   rd          rate-distortion pruning, goal FIC_QT_RD_LAMBDA / _LEAVES / _SSE for all planes, values[p] as `value` above
 * All ranges are checked for every plane before any launch; FIC_E_STATE without an input. */
FIC_API int fic_qt_ctx_encode_threshold(fic_qt_ctx* ctx, const float* thresholds, void* hip_stream);
FIC_API int fic_qt_ctx_encode_budget(fic_qt_ctx* ctx, const int64_t* max_leaves, void* hip_stream);
FIC_API int fic_qt_ctx_encode_rd(fic_qt_ctx* ctx, int goal, const uint64_t* values, void* hip_stream);
FIC_API int fic_qt_ctx_sync(fic_qt_ctx* ctx);
/* Results of the last encode (the host getters wait for it).  n_leaves int32 [planes]; param uint32 [planes]: the bits of the
 * threshold (threshold and budget rules) or lambda in force; stats uint64 [planes][4] as stats4 above.  Any may be NULL. */
FIC_API int fic_qt_ctx_get_results_host(fic_qt_ctx* ctx, int32_t* n_leaves, uint32_t* param, uint64_t* stats);
/* The leaf table of one plane, rows of 7 (grey) or 9 (colour) ints; *n_leaves is set on FIC_E_CAPACITY too. */
FIC_API int fic_qt_ctx_get_leaves_host(fic_qt_ctx* ctx, int plane, int32_t* leaves, int64_t capacity, int* n_leaves);
/* Device pointers of the same, stable for the life of the context: leaves int32 [planes][(w / B_min) * (h / B_min)][7 or 9]
 * (a fixed stride per plane; the rows of a plane beyond its n_leaves are unspecified), n_leaves, param, stats as above. */
FIC_API int fic_qt_ctx_result_device_ptrs(fic_qt_ctx* ctx, void** leaves, void** n_leaves, void** param, void** stats);
/* Decode and collage of every plane of the last encode at once, from the tables as they stand on the device
 * -- leaves and n_leaves above, the context's geometry, wK and n_iso -- never through a stream or the host.
 *   out      [planes][zoom h][zoom w]: uint8_t for a grey context, packed int32_t ARGB for a colour one; capacity_pixels counts
 *            the pixels of all planes
 *   decode   zoom 1, 2 or 4 (every leaf {x, y, B} painted as {zoom x, zoom y, zoom B}); plane p is, bit for bit, what
 *            fic_decode_quadtree_run_zoom (grey) / fic_decode_rgb_quadtree_iso_run (colour) returns for plane p's stream at
 *            that zoom with avgError 0 carried in: the image, avg_error_out[p], iterations_out[p] (either may be NULL)
 *   collage  plane p is one paint of its leaves from the 2:1 copy of the input image: the image whose squared distance from the
 *            input, summed over a leaf, is that leaf's collage SSE, and over the plane stats[p][0]
 * FIC_E_ARGUMENT for a null argument or a zoom outside {1, 2, 4}, FIC_E_STATE before the first encode, FIC_E_CAPACITY when out
 * is too small, FIC_E_GEOMETRY for a block side above 64 at that zoom; FIC_E_ARGUMENT, naming the plane, when a plane's table
 * on the device is no longer a tiling of the image by valid rows (the caller can write it): nothing is read through such a row,
 * `out` is not written, and the context takes the next encode as ever.  Both wait for the last encode's stream. */
FIC_API int fic_qt_ctx_decode_zoom_host(fic_qt_ctx* ctx, int zoom, void* out, int64_t capacity_pixels, float* avg_error_out,
                                        int* iterations_out);
FIC_API int fic_qt_ctx_collage_host(fic_qt_ctx* ctx, void* out, int64_t capacity_pixels);

/* Tuning / instrumentation knobs:
 *   "sweep"       0 auto: windowed search -> generic kernel; full search -> the VALU sweep (k_sweep_d4, the
 *                     group-Fourier form, for 8 isometries at B = 8; k_sweep_fast otherwise)
 *                 1 generic, 2 k_sweep_fast (VALU, v_dot4), 5 k_sweep_d4 (VALU, v_dot2c; n_iso = 8, B = 8 only),
 *                 3 = opt-in matrix-core sweep (B = 4/8/16, n_iso = 1 or 8, full search; same results): bf16
 *                     operands (centred pixels are exact bf16) at B = 4/8 and at B = 16 with 8 isometries, i8
 *                     operands at B = 16 with 1 isometry -- whichever is faster
 *                 4 = matrix-core sweep with i8 operands at every block size (the round's first kernels; kept)
 *                 6 = the DEFAULT full-search sweep k_sweep_q (fic_q.hip): f16 matrix-core prune GEMM on a normalised domain
 *                     operand + exact evaluation of the surviving pairs (B = 4/8/16, n_iso = 1 or 8)
 *                 (with "sweep" = 0 the environment variable FIC_SWEEP=3 selects the matrix-core sweep process-wide
 *                 for full-search launches of >= 5e7 (B = 4/8) / 5e8 (B = 16) (range, domain) pairs; smaller
 *                 launches and windowed search keep the VALU sweep, which is faster there)
 *   "q_shape"     matrix instruction of the 1-isometry k_sweep_q at B = 8 / 16: 0 by pool size (default: v_mfma_f32_16x16x32_f16
 *                 from 10^5 K-steps per range column, else 32x32x16), 1 = 16x16x32 (k_sweep_q16), 2 = 32x32x16; same codebooks
 *   "q_eshift"    diagnostic, -12..4 (default 0): k_sweep_q stores its per-range error bound E_r times 2^-q_eshift.  Negative
 *                 values widen the prune threshold (more pairs evaluated exactly, same codebooks); positive values narrow it
 *                 below what the derivation in fic_q.hip allows and give WRONG codebooks (the tests show that they are caught).
 *                 Like "q_noflag", not for production use.  fic_rgb_ctx_set_option takes it too (matrix-core RGB sweep).
 *   "search"      0 (default) the reference's criterion (getErrorVarianceCovariance), 1 the least-squares search described at
 *                 fic_encode_gray_lsq_u8 below.  Under "search" = 1, "sweep" takes 0 (auto: k_sweep_lsq_generic for windows,
 *                 k_sweep_lsq_fast for full search), 1 (generic) or 2 (fast, full search only); any other value is
 *                 FIC_E_ARGUMENT, whichever of the two options is set last.  "chunks", range spans, batched planes,
 *                 "time_sweep" and fic_ctx_last_kernel work as with "search" = 0, and so do fic_ctx_collage_host and
 *                 fic_ctx_decode_host / fic_ctx_decode_zoom_host: a and b are the decoder's own values then.
 *   "lsq_tau_widen"  diagnostic, 0 (off, the default) or 8..24: k_sweep_lsq_fast multiplies the tau of its prune bound by
 *                 1 + 2^-value after the safety factor, above what the derivation in fic_lsq.hip allows: > 0 gives WRONG
 *                 codebooks (the tests show that they are caught).  Not for production use; the contexts behind the one-shot
 *                 entries never carry it.  fic_rgb_ctx_set_option takes it too (k_sweep_lsq_rgb_fast).
 *   "lsq_engine"  0 (default) or 1; any other value is FIC_E_ARGUMENT and leaves the option as it was.  Under 1, an encode under
 *                 "search" = 1 that would have launched k_sweep_lsq_fast (full search with "sweep" 0 or 2) launches the
 *                 matrix-core sweep k_sweep_lsq_q instead: an f16 GEMM decides which pairs can be
 *                 skipped, every other pair is evaluated by the integer arithmetic of k_sweep_lsq_fast -- the same codebooks,
 *                 bit for bit.  "sweep" = 1, windowed searches and "search" = 0 are untouched.  "chunks" then counts pool
 *                 chunks in domain tiles of 32 blocks; range spans, batched planes, "time_sweep", the collage and the decodes
 *                 work as before.  The one-shot and quadtree entries (and their cached contexts) never use it.
 *   "lsq_q_eshift"  diagnostic, -12..4 (default 0): k_sweep_lsq_q's per-range rounding allowance Er is stored times 2^-value.
 *                 Negative values widen the bound (more pairs evaluated exactly, same codebooks); positive values narrow it
 *                 below what the derivation in fic_lsq_q.hip allows and give WRONG codebooks (the tests show that they are
 *                 caught).  Not for production use.  "lsq_tau_widen" applies to k_sweep_lsq_q's theta as it does to tau.
 *   "chunks"      domain-pool chunks per range tile for the fast kernel (0 = auto)
 *   "time_sweep"  1: bracket every sweep launch with hipEvents on its stream */
FIC_API int fic_ctx_set_option(fic_ctx* ctx, const char* name, int value);

/* ---- least-squares domain search (an extension) ------------------------------------------------------
 * The reference picks the domain block by rem^2 (1 - r^2) (getErrorVarianceCovariance, FractalCompression.java:655-687), clamps
 * a afterwards and truncates (int)(a*100), (int) b in writeData.  This search minimises the squared error of the QUANTISED map
 * the decoder will paint, in exact integers -- no float decides anything.  Same pool, same window, same 8 isometries, same
 * streams and decoders; only the choice and the coefficients differ.  For range block r and candidate d = pool block g read
 * through isometry k (n = B*B):
 *   S_r = sum r, S_rr = sum r^2, S_d = sum d, S_dd = sum d^2, S_rd = sum r d_k;   C = n S_rd - S_r S_d,  V = n S_dd - S_d^2
 *   qa = 0 if V == 0, else clamp(floor((200 C + V) / (2 V)), -100, 100)      (100 C / V to nearest, then the clamp; floor is
 *                                                                             the mathematical one, also for negatives)
 *   qb = floor((2 (100 S_r - qa S_d) + 100 n) / (200 n))                     (mean_r - qa mean_d / 100 to nearest, not clamped)
 *   E  = sum (100 r - qa d - 100 qb)^2 = 10^4 S_rr + qa^2 S_dd + 10^4 n qb^2 - 200 qa S_rd - 2 10^4 qb S_r + 200 qa qb S_d
 * (int64, >= 0: 10^4 times the squared error of the quantised map before the decoder's truncation and pixel clamp).  The winner
 * is the smallest E; candidates in the order c = idx_local * n_iso + k, strict '<' (the first candidate wins a tie).  Outputs:
 *   idx_local, iso   the winner;   qrows = {idx_local, qa, qb} as they are (no (int)(a*100) step)
 *   a = (float) qa / 100f, b = (float) qb   (what decodeGreyScale makes of the row, :373);   err = (float)((double) E / 1e4)
 *   E [planes][N_r]  fic_ctx_get_lsq_error_host after an encode with "search" = 1 (FIC_E_STATE otherwise)
 * The one-shot entries take the arguments of fic_encode_gray_u8 / _argb plus E [N_r], which may be NULL, and run through the same
 * cached contexts; a context goes back to the cache in the reference's mode.  The quadtree entries have the signature of
 * fic_encode_gray_quadtree_u8 / _argb: the per-level codebooks come from this search, everything after them (leaf SSE, split,
 * leaf table, tag-2 stream, decoder) is unchanged. */
FIC_API int fic_ctx_get_lsq_error_host(fic_ctx* ctx, int64_t* E);
FIC_API int fic_encode_gray_lsq_u8(const uint8_t* gray, int w, int h, int B, int wK, int n_iso, int device, int32_t* idx_local,
                                   float* a, float* b, int32_t* iso, int32_t* qrows, int64_t* E);
FIC_API int fic_encode_gray_lsq_argb(const int32_t* argb, int w, int h, int B, int wK, int n_iso, int device, int32_t* idx_local,
                                     float* a, float* b, int32_t* iso, int32_t* qrows, int64_t* E);
FIC_API int fic_encode_gray_quadtree_lsq_u8(const uint8_t* gray, int w, int h, int B_max, int B_min, int wK, int n_iso, float threshold,
                                            int device, int32_t* leaves, int64_t capacity, int* n_leaves);
FIC_API int fic_encode_gray_quadtree_lsq_argb(const int32_t* argb, int w, int h, int B_max, int B_min, int wK, int n_iso,
                                              float threshold, int device, int32_t* leaves, int64_t capacity, int* n_leaves);
/* ---- least-squares domain search, joint RGB (an extension) --------------------------------------------
 * The reference's colour criterion (getErrorVarianceCovarianceRGB, FractalCompression.java:760-808) works on the sum of the
 * three channels, divides by varianceR + varianceG + mittelWertB, never sets the domain variance and clamps a after the winner
 * is chosen.  This search minimises, in exact integers, the squared error over the three channels of the QUANTISED map -- one
 * a, three b, as in the reference's row.  Same pool (createCodebuchRGB), window, isometries, streams and decoders.  Per channel
 * ch in {R, G, B}: S_r, S_rr, S_d, S_dd, S_rd = sum r d_k (n = B*B);
 *   C = sum_ch (n S_rd - S_r S_d),   V = sum_ch (n S_dd - S_d^2)
 *   qa = 0 if V == 0, else clamp(floor((2000 C + V) / (2 V)), -1000, 1000)          (1000 C / V to nearest, then the clamp)
 *   t_R, t_G = floor((2 (1000 S_r - qa S_d) + 10 n) / (20 n))                       (100 (mean_r - a mean_d) to nearest)
 *   t_B      = floor((2 (1000 S_r - qa S_d) + 1000 n) / (2000 n))                   (the stream's bB is an integer)
 *   u = {10 t_R, 10 t_G, 1000 t_B};   E = sum_ch sum_i (1000 r - qa d - u_ch)^2     (int64, >= 0, < 2^50)
 * The winner is the smallest E; candidates in the order c = idx_local * n_iso + k, strict '<'.  Outputs: idx_local, iso;
 * qrows5 = {idx_local, 1000 qa, 1000 t_R, 1000 t_G, t_B}, which every writer and decoder of colour rows takes unchanged;
 * a, bR, bG, bB what decodeRGB makes of that row ((float) q1 / 1e6f, (float) q2 / 1e5f, (float) q3 / 1e5f, (float) q4), so the
 * collage and the context's decode need no change; E [planes][N_r] through fic_rgb_ctx_get_lsq_error_host (FIC_E_STATE unless
 * the last encode was a least-squares one).
 * fic_rgb_ctx_set_option(ctx, "search", 0 | 1) switches a colour context.  Under "search" = 1, "sweep" means 0 (auto:
 * k_sweep_lsq_rgb_fast for full search at B <= 8, else k_sweep_lsq_rgb_generic), 1 (generic) or 2 (fast; an encode of any other
 * geometry returns FIC_E_ARGUMENT); FIC_RGB_SWEEP does not apply.  "chunks" (pool chunks of the fast sweep, 0 = auto), batched
 * planes, fic_rgb_ctx_last_kernel, the collage and fic_rgb_ctx_decode_host / _zoom_host work as before; "sweep_stats" counts as
 * under the grey search (fic_ctx_sweep_stats).  fic_encode_rgb_lsq_argb takes the arguments of fic_encode_rgb_iso_argb plus
 * E [N_r] (may be NULL) and runs over the same cached contexts, which go back to the cache in the reference's mode.  The two
 * quadtree entries have the signatures of fic_encode_rgb_quadtree_argb (tag 3) and fic_encode_rgb_quadtree_iso_argb (tag 6):
 * the per-level codebooks come from this search, everything after them is unchanged. */
FIC_API int fic_rgb_ctx_get_lsq_error_host(fic_rgb_ctx* ctx, int64_t* E);
/* The same search on the matrix cores, options of a colour context:
 *   "lsq_engine"    0 (default: today's sweeps, launch for launch) or 1; any other value is FIC_E_ARGUMENT and leaves the option
 *                   as it was, whatever else is set.  Under 1, an encode under "search" = 1 with full search (wK == Dw == Dh),
 *                   "sweep" 0 or 2, B = 4 / 8 / 16 and 1 or 8 isometries launches k_sweep_lsq_rgb_q<NK, CSHIFT> (NK = 3 n / 16 =
 *                   3, 12, 48; CSHIFT = 0 or 3): where k_sweep_lsq_rgb_fast would run at B <= 8, and where the automatic choice
 *                   would take k_sweep_lsq_rgb_generic at B = 16.  "sweep" = 2 at B = 16 stops being refused only under this
 *                   option.  An f16 GEMM over the 3 n entries of a block decides which pairs can be skipped; every other pair is
 *                   evaluated as before: the codebook and E are the same bits.  "sweep" = 1, windows and "search" = 0 never see
 *                   the option; the one-shot, quadtree and leaf-budget entries and their cached contexts never set it.  "chunks"
 *                   then counts pool chunks in domain tiles of 32 blocks (0 = automatic).  fic_rgb_ctx_last_kernel reports the
 *                   kernel; "sweep_stats" counts out[0] tile epilogues (32 columns x 32 pool blocks), out[1] tiles with flagged
 *                   pairs, out[2] pairs evaluated exactly, out[3] waves.
 *   "lsq_q_eshift"  diagnostic, -12..4 (default 0): that sweep's per-range rounding allowance Er is stored times 2^-value.
 *                   Values > 0 put it below what the derivation in fic_lsq_rgb_q.hip allows and give WRONG codebooks.  Not for
 *                   production use.  "lsq_tau_widen" acts on that sweep's tau as on k_sweep_lsq_rgb_fast's.
 *   "time_sweep"    1: bracket the sweep launch of every encode under "search" = 1 with hipEvents on its stream (with 0, the
 *                   default, no event is created); fic_rgb_ctx_sweep_time reads them as fic_ctx_sweep_time does.
 * fic_rgb_ctx_last_lsq_chunks: pool chunks of the last least-squares sweep (0: the last encode was none). */
FIC_API int fic_rgb_ctx_sweep_time(fic_rgb_ctx* ctx, double* total_ms, int* launches, int reset);
FIC_API int fic_rgb_ctx_last_lsq_chunks(fic_rgb_ctx* ctx);
FIC_API int fic_encode_rgb_lsq_argb(const int32_t* argb, int w, int h, int B, int wK, int n_iso, int device, int32_t* idx_local,
                                    float* a, float* bR, float* bG, float* bB, int32_t* iso, int32_t* qrows5, int32_t* collage_argb,
                                    int64_t* E);
FIC_API int fic_encode_rgb_quadtree_lsq_argb(const int32_t* argb, int w, int h, int B_max, int B_min, int wK, float threshold,
                                             int device, int32_t* leaves, int64_t capacity, int* n_leaves);
FIC_API int fic_encode_rgb_quadtree_iso_lsq_argb(const int32_t* argb, int w, int h, int B_max, int B_min, int wK, int n_iso,
                                                 float threshold, int device, int32_t* leaves, int64_t capacity, int* n_leaves);
/* Sum of sweep-kernel durations (ms) and launch count since the last reset ("time_sweep" = 1).
 * Synchronises the events.  reset != 0 clears the accumulators afterwards. */
FIC_API int fic_ctx_sweep_time(fic_ctx* ctx, double* total_ms, int* launches, int reset);
/* Counters of the default sweep k_sweep_q since the last reset (option "sweep_stats" = 1 first): out[0] tile epilogues
 * (32 range copies x 32 domain blocks each), out[1] tiles that had flagged pairs, out[2] pairs evaluated exactly,
 * out[3] waves; of a sample of the waves: out[4] shader-clock cycles and out[5] 100 MHz ticks they were alive (summed),
 * out[6] their number (out[4] / out[5] / 10 = the clock in GHz the chip held under this kernel); out[7] reserved.
 * Under "search" = 1 the fast sweep k_sweep_lsq_fast counts instead: out[0] (wave, pool block) visits, out[1] visits that ran
 * the exact epilogue (some lane had a pair the prune could not skip), out[2] pairs evaluated exactly, out[3] waves.
 * Under "lsq_engine" = 1 k_sweep_lsq_q counts with k_sweep_q's meaning: out[0] tile epilogues (32 columns x 32 pool blocks
 * each), out[1] tiles that had flagged pairs, out[2] pairs evaluated exactly, out[3] waves; out[4..7] stay 0.
 * Synchronises the context's stream. */
FIC_API int fic_ctx_sweep_stats(fic_ctx* ctx, uint64_t* out8, int reset);
/* Geometry actually in use: out[0..9] = Rw, Rh, N_r, Dw, Dh, N_d, NR, tiles, chunks, sweep kind.  The sweep kind is the value
 * of "sweep" that ran (1..6; under "search" = 1: 1 generic, 2 fast), or 7: the matrix-core least-squares sweep k_sweep_lsq_q
 * ("lsq_engine" = 1). */
FIC_API int fic_ctx_info(fic_ctx* ctx, int* out10);
/* Name of the sweep kernel the context's last encode launched (as rocprofv3 prints it, without the argument list), e.g.
 * "k_sweep_lsq_fast" / "k_sweep_lsq_generic" under "search" = 1 ("lsq_engine" = 1: "k_sweep_lsq_q<NK, CSHIFT>" with NK = n / 16 =
 * 1, 4, 16 and CSHIFT = 0 (1 isometry) or 3 (8 isometries), e.g. "k_sweep_lsq_q<4, 3>"), "k_sweep_q<4, 2, false>" (one pool chunk), "k_sweep_q16<4, true>" (several) or "k_sweep_qs<4, 2>" / "k_sweep_q16s<4>" (several short
 * ones: theta is shared between the chunks in the fast path) -- so that a caller can match its timing with a profile.  A small launch
 * of the default sweep (one image up to about 512x512 at B = 8) runs as two kernels instead of five -- k_prep_q8 (scale + pool +
 * range prep) and the sweep, whose last workgroup per range-column group also does k_finalize's work -- and the name then
 * carries the suffix " after k_prep_q8, finalising". */
FIC_API int fic_ctx_last_kernel(fic_ctx* ctx, char* out, int capacity);
/* Range blocks one wave of sweep `kind` keeps in registers, i.e. how many range blocks share one read of a pool block
 * (the reuse factor between SURVEY 8(d)'s byte model and the physical traffic): k_sweep_q 32 / 128 (B = 8: 8 / 1
 * isometries), 32 / 256 (B = 4), 16 / 64 (B = 16); the VALU sweeps 64 x NR.  0: not defined for that kind. */
FIC_API int fic_sweep_ranges_per_pool_read(int kind, int B, int n_iso);

/* Test hook: out[i] = sqrt((double)(first + i)) computed on the device exactly as the pool
 * kernel does for Domainblock.variance (FractalCompression.java:677,680 Math.sqrt). */
FIC_API int fic_debug_sqrt_f64(int device, uint32_t first, uint32_t count, double* out);
/* Test hook: out[0] = the decoder's reproduction of Java's loop `avg = carry; for (i) avg += (float) vals[i];`
 * (FractalCompression.java:407) on the device. */
FIC_API int fic_debug_float_sum(int device, float carry, const uint32_t* vals, int count, float* out);
/* Segments (65 536 values) of this thread's last fic_debug_float_sum whose sum left its binade (or had a fractional carry-in)
 * and therefore took the sequential-order path instead of the precomputed segment map. */
FIC_API int fic_debug_float_sum_fallbacks(void);
/* Test hook: fic_decode_gray_run that also reports in seq_sums how many iterations took the sequential float sum. */
FIC_API int fic_debug_decode_gray_run(const uint8_t* run, int64_t len, int device, uint8_t* gray_out, int64_t capacity,
                                      float* avg_error_io, int* iterations, int* seq_sums);
/* Test hook: loads RCCL, creates one communicator per device 0..|n|-1 and (|n| >= 2) runs the codebook gather's grouped
 * send/recv pattern on dummy records, checking what arrives on device 0.  n < 0: the gather's ERROR path on |n| devices
 * (a send to a peer that does not exist must fail, leave no group open and no communicator cached; the same pattern
 * must then succeed on fresh communicators). */
FIC_API int fic_debug_rccl_selftest(int n);
/* Calls of fic_encode_gray_*_multi in this process that finished with peer copies after an RCCL failure (FIC_GATHER
 * unset / "rccl": fall back; "rccl-only": return the error; "copy": peer copies only). */
FIC_API int fic_debug_gather_fallbacks(void);
/* Test hook: copies the pool of the last encode to the host: pix u8 [planes][N_d][n],
 * sum u32 [planes][N_d], var u32 [planes][N_d], scaled u8 [planes][h/2][w/2]. NULLs allowed. */
FIC_API int fic_ctx_debug_pool_host(fic_ctx* ctx, uint8_t* pix, uint32_t* sum, uint32_t* var, uint8_t* scaled);
/* Test hook: raw bytes of one store of the default sweep k_sweep_q after an encode through it, as the prep kernels left them:
 * which = 0 A fragments [planes][domain tiles + padding][NK][64] x 8 f16, 1 flat-tile flags u32 [planes][domain tiles + padding],
 * 2 B fragments [planes][column tiles + padding][NK][64] x 8 f16, 3 E_r f32 [planes][padded N_r], 4 range statistics
 * {rM, rem} i32 pairs [planes][padded N_r], 5 the columns' copies as bytes [planes][padded N_r][columns per range][n].
 * *size = the store's size in bytes; out may be NULL (size only), else capacity must hold it. */
FIC_API int fic_ctx_debug_q_host(fic_ctx* ctx, int which, void* out, int64_t capacity, int64_t* size);
/* Test hook: raw bytes of one store of k_lsq_q_prep after an encode through k_sweep_lsq_q ("search" = 1, "lsq_engine" = 1;
 * FIC_E_STATE before the first one): which = 0 A fragments [planes][domain tiles][NK][64] x 8 f16 (slot (m, lane): elements
 * [16 m + 8 (lane >> 5), +8) of pool block 32 tile + (lane & 31)), 1 B fragments [planes][column tiles][NK][64] x 8 f16 (column
 * = range block * n_iso + isometry), 2 the allowance Er f32 [planes][padded N_r], 3 R = n S_rr - S_r^2 u32 [planes][padded N_r].
 * *size = the store's size in bytes; out may be NULL (size only), else capacity must hold it. */
FIC_API int fic_ctx_debug_lsq_q_host(fic_ctx* ctx, int which, void* out, int64_t capacity, int64_t* size);
/* Test hook, joint RGB: the same for the matrix-core RGB sweep ("sweep" = 2) of the LAST plane encoded: which = 0 A fragments
 * [domain tiles + padding][NK][64] x 8 f16, 1 flat-tile flags, 2 B fragments [column tiles + padding][NK][64] x 8 f16, 3 E_r f32 [N_r],
 * 4 {0, varianzRange} i32 pairs [N_r], 5 Amax (f32 bits, one u32).  On an n_iso = 8 context the B fragments hold 8 adjacent
 * columns per range block, column 8 j + k the copy c_k of range j with c_k[src_k(i)] = greyR[i]; the other stores are unchanged. */
FIC_API int fic_rgb_ctx_debug_q_host(fic_rgb_ctx* ctx, int which, void* out, int64_t capacity, int64_t* size);
/* Test hook, joint RGB: raw bytes of one store of k_lsq_rgb_q_prep after an encode through k_sweep_lsq_rgb_q ("search" = 1,
 * "lsq_engine" = 1; FIC_E_STATE before the first one), as fic_ctx_debug_lsq_q_host with NK = 3 n / 16 and element i = ch * n + pos
 * of a block: which = 0 A fragments [planes][domain tiles][NK][64] x 8 f16, 1 B fragments [planes][column tiles][NK][64] x 8 f16,
 * 2 the allowance Er f32 [planes][N_r padded to 64], 3 R = n S_rr - sum_ch S_r^2 u32 [planes][N_r padded to 64]. */
FIC_API int fic_rgb_ctx_debug_lsq_q_host(fic_rgb_ctx* ctx, int which, void* out, int64_t capacity, int64_t* size);

/* Test hook: what the library holds right now, process-wide, through contexts, the one-shot caches, the decoders' arenas and
 * any call in flight: out4 = {device bytes, device allocations, pinned host bytes, pinned host allocations}.  All four are 0
 * once every context is destroyed and fic_release_cache() has run.  Needs no device. */
FIC_API int fic_debug_live_memory(int64_t out4[4]);

#ifdef __cplusplus
}
#endif
#endif /* FIC_H */
