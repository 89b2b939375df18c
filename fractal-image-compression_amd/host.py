"""Host-side mirror of the reference's interface for the grey encode path.

Same names, argument meaning and error behaviour as bvk_ss19 (src/bvk_ss19/):
  RasterImage           RasterImage.java:18-24   public fields argb, width, height
  FractalCompression    FractalCompression.java  statics blockgroesse (:14), widthKernel (:15),
                        encode (:54), encodeGrayScale (:109), isGreyScale (:32), writeData (:230),
                        getBestGeneratedCollage (:269)
All block search runs in libfic_hip.so on the GPU (capi.py); nothing here computes a match.
"""
import ctypes as C
import io

import numpy as np

from . import capi
from .capi import FicError


class RasterImage:
    """RasterImage.java:18-24 -- int[] argb (ARGB, scanline order), width, height."""

    def __init__(self, width, height, argb=None):
        self.width = int(width)
        self.height = int(height)
        if argb is None:
            argb = np.zeros(self.width * self.height, np.int32)          # new int[w*h]
        self.argb = np.ascontiguousarray(argb, np.int32).reshape(-1)
        if self.argb.size != self.width * self.height:
            raise ValueError("argb has the wrong number of pixels")

    @classmethod
    def from_gray(cls, gray):
        g = np.ascontiguousarray(gray, np.uint8)
        u = g.astype(np.uint32)
        argb = (0xFF000000 | (u << 16) | (u << 8) | u).astype(np.uint32).view(np.int32)
        return cls(g.shape[1], g.shape[0], argb.reshape(-1))

    def red(self):
        return ((self.argb.view(np.uint32) >> 16) & 0xFF).astype(np.uint8).reshape(self.height, self.width)


class _DevArray:
    """Exposes a raw device pointer through __cuda_array_interface__ so torch can alias it."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False),
                                         "version": 2, "strides": None}


class Encoder(capi.Handle):
    """Handle API (fic_ctx_*): the working set for `planes` grey images of one geometry on one
    device.  Inputs may be numpy arrays (copied to the device) or torch CUDA tensors (used in
    place: this is what bench.py times).

    Options (set_option, fic_ctx_set_option): "search" also takes "reference" / "lsq" (least squares).
    "lsq_tau_widen": 0 (off) or 8..24 -- diagnostic, > 0 gives WRONG codebooks (the fast least-squares sweep's bound times
    1 + 2^-value).  "lsq_engine": 0 / "valu" (k_sweep_lsq_fast) or 1 / "mfma" (the matrix-core sweep k_sweep_lsq_q, DESIGN.md
    4.21: the same codebooks); "lsq_q_eshift": -12..4, diagnostic, > 0 gives WRONG codebooks (that sweep's allowance times
    2^-value)."""

    PREFIX = "fic_ctx"

    def __init__(self, width, height, B, wK=None, n_iso=1, planes=1, device=0):
        L = capi.lib()
        self.width, self.height, self.B, self.n_iso, self.planes, self.device = width, height, B, n_iso, planes, device
        Rw, Rh, Dw, Dh = capi.geometry(width, height, B)
        if wK is None:
            if Dw != Dh:
                raise FicError(-2, "full search (wK=None) needs a square block grid, as in the reference (FC:89-96)")
            wK = Dw
        self.wK = wK
        self.Rw, self.Rh, self.Dw, self.Dh = Rw, Rh, Dw, Dh
        self.n_ranges, self.n_domains = Rw * Rh, Dw * Dh
        self._encode, = self._open(L.fic_ctx_create(device, width, height, B, wK, n_iso, planes), "encode")
        self.ranges_per_tile = 64 * self.info()["NR"]

    # ---- input -----------------------------------------------------------------------------
    def set_gray(self, gray):
        """gray: uint8 [planes,H,W] / [H,W] numpy array (copied), or a torch CUDA uint8 tensor of that shape.  A tensor whose
        address is a multiple of 8 is used in place and read by every later encode, at encode time; any other one (a view at
        an odd offset) is cloned here, once, into a fresh allocation: later writes to it are not seen."""
        if hasattr(gray, "data_ptr"):                                  # torch tensor, device resident
            return self._set_device(gray, 1, 8, "set_gray_device", "uint8")
        g = np.ascontiguousarray(gray, np.uint8)
        n = self.planes * self.height * self.width
        if g.size != n:
            raise FicError(-3, f"input has {g.size} pixels, expected {n}")
        capi.check(capi.lib().fic_ctx_set_gray_host(self._h, capi.ptr(g, C.c_uint8)))

    def set_argb(self, argb):
        a = np.ascontiguousarray(argb, np.int32)
        if a.size != self.planes * self.height * self.width:
            raise FicError(-3, "argb has the wrong number of pixels")
        capi.check(capi.lib().fic_ctx_set_argb_host(self._h, capi.ptr(a, C.c_int32)))

    # ---- compute ---------------------------------------------------------------------------
    def encode(self, range_begin=0, range_count=-1, stream=None):
        """Asynchronous on `stream` (a raw hipStream_t handle / torch stream, None = default)."""
        capi.check(self._encode(self._h, range_begin, range_count, self._stream(stream)))

    def sweep_stats(self, reset=True):
        """k_sweep_q counters (after set_option("sweep_stats", 1)): tile epilogues, flagged tiles, exact pairs, waves,
        and of a sample of the waves the shader-clock cycles / 100 MHz ticks they lived (`clock_ghz` = their ratio)."""
        d = super().sweep_stats(reset)
        d["clock_ghz"] = d["wave_cycles"] / d["wave_ticks"] / 10.0 if d["wave_ticks"] else None
        return d

    def info(self):
        v = (C.c_int * 10)()
        capi.check(capi.lib().fic_ctx_info(self._h, v))
        keys = ["Rw", "Rh", "Nr", "Dw", "Dh", "Nd", "NR", "tiles", "chunks", "sweep_kind"]
        return dict(zip(keys, list(v)))

    # ---- results ---------------------------------------------------------------------------
    def results(self):
        P, N = self.planes, self.n_ranges
        r = {
            "idx_local": np.zeros((P, N), np.int32), "a": np.zeros((P, N), np.float32),
            "b": np.zeros((P, N), np.float32), "iso": np.zeros((P, N), np.int32),
            "qrows": np.zeros((P, N, 3), np.int32), "idx_global": np.zeros((P, N), np.int32),
            "err": np.zeros((P, N), np.float32),
        }
        capi.check(capi.lib().fic_ctx_get_results_host(
            self._h, capi.ptr(r["idx_local"], C.c_int32), capi.ptr(r["a"], C.c_float), capi.ptr(r["b"], C.c_float),
            capi.ptr(r["iso"], C.c_int32), capi.ptr(r["qrows"], C.c_int32), capi.ptr(r["idx_global"], C.c_int32),
            capi.ptr(r["err"], C.c_float)))
        return r

    def results_device(self):
        """torch tensors aliasing the context's device result arrays (no copy)."""
        import torch
        p = [C.c_void_p() for _ in range(7)]
        capi.check(capi.lib().fic_ctx_result_device_ptrs(self._h, *[C.byref(x) for x in p]))
        P, N = self.planes, self.n_ranges
        dev = torch.device("cuda", self.device)

        def t(ptr, shape, ts):
            return torch.as_tensor(_DevArray(ptr.value, shape, ts), device=dev)

        return {"idx_local": t(p[0], (P, N), "<i4"), "a": t(p[1], (P, N), "<f4"), "b": t(p[2], (P, N), "<f4"),
                "iso": t(p[3], (P, N), "<i4"), "qrows": t(p[4], (P, N, 3), "<i4"),
                "idx_global": t(p[5], (P, N), "<i4"), "err": t(p[6], (P, N), "<f4")}

    def records_device(self):
        """torch int32 tensor [planes, N_r, 6] aliasing the context's packed codebook records (the unit of the gather)."""
        import torch
        p = C.c_void_p()
        capi.check(capi.lib().fic_ctx_records_device_ptr(self._h, C.byref(p)))
        return torch.as_tensor(_DevArray(p.value, (self.planes, self.n_ranges, 6), "<i4"), device=torch.device("cuda", self.device))

    def collage(self):
        out = np.zeros((self.planes, self.height * self.width), np.int32)
        capi.check(capi.lib().fic_ctx_collage_host(self._h, capi.ptr(out, C.c_int32)))
        return out

    def decode(self, zoom=1):
        """Reference decoder loop (FC:356-421) on the device from the last encode's quantised rows
        (+ isometries).  Returns (gray uint8 [planes,H,W], avgError float32 [planes], iterations int32 [planes]).
        zoom = 2 / 4: the same loop on the geometry (zoom*W, zoom*H, zoom*B, wK), [planes, zoom*H, zoom*W] out
        (fic_ctx_decode_zoom_host)."""
        P = self.planes
        avg = np.zeros(P, np.float32)
        it = np.zeros(P, np.int32)
        if zoom != 1:
            z = int(zoom) if zoom in (1, 2, 4) else 1     # the library refuses any other zoom before it writes
            out = np.zeros((P, z * self.height, z * self.width), np.uint8)
            capi.check(capi.lib().fic_ctx_decode_zoom_host(self._h, int(zoom), capi.ptr(out, C.c_uint8), capi.ptr(avg, C.c_float),
                                                           capi.ptr(it, C.c_int)))
            return out, avg, it
        out = np.zeros((P, self.height, self.width), np.uint8)
        capi.check(capi.lib().fic_ctx_decode_host(self._h, capi.ptr(out, C.c_uint8), capi.ptr(avg, C.c_float),
                                                  capi.ptr(it, C.c_int)))
        return out, avg, it

    def debug_pool(self):
        P, Nd, n = self.planes, self.n_domains, self.B * self.B
        pix = np.zeros((P, Nd, n), np.uint8)
        s = np.zeros((P, Nd), np.uint32)
        v = np.zeros((P, Nd), np.uint32)
        sc = np.zeros((P, self.height // 2, self.width // 2), np.uint8)
        capi.check(capi.lib().fic_ctx_debug_pool_host(self._h, capi.ptr(pix, C.c_uint8), capi.ptr(s, C.c_uint32),
                                                      capi.ptr(v, C.c_uint32), capi.ptr(sc, C.c_uint8)))
        return {"pix": pix, "sum": s, "var": v, "scaled": sc}

    Q_STORES = ("pool", "flat", "rng", "E", "rng_st", "rngC")
    LSQ_Q_STORES = ("A", "B", "Er", "R")

    def debug_lsq_q(self, which):
        """Raw bytes (uint8 array) of one store of k_lsq_q_prep after an encode through k_sweep_lsq_q ("lsq_engine" = 1): "A" /
        "B" the fragments, "Er" the per-range allowance (f32), "R" (u32) (fic_ctx_debug_lsq_q_host; tests/lsqqmodel.py decodes them)."""
        return self._debug_store("debug_lsq_q_host", self.LSQ_Q_STORES, which)

    def debug_q(self, which):
        """Raw bytes (uint8 array) of one store of k_sweep_q after an encode through it ("sweep" = 6): "pool" / "rng" the
        A / B fragments, "flat" the flat-tile flags, "E" the per-range error bounds, "rng_st" {rM, rem} per range, "rngC" the
        columns' copies as bytes (fic_ctx_debug_q_host; tests/qmodel.py decodes them)."""
        return self._debug_store("debug_q_host", self.Q_STORES, which)


class QuadtreeEncoder(capi.Handle):
    """Handle API of the quadtree codec (fic_qt_ctx_*): `planes` images of one geometry, every split rule, device
    resident and asynchronous like Encoder.  colour=False: grey, leaf rows of 7 ints (write_run_quadtree); colour=True: joint RGB
    with the isometry column, rows of 9 ints (write_run_rgb_quadtree_iso), n_iso 1 or 8.  wK = 0: full search at every level.
    Plane p's results are those of the one-shot entry (encode_gray_quadtree*, encode_rgb_quadtree_iso*) on image p.
    set_option: "search", "reference" / 0 or "lsq" / 1, the criterion of the per-level codebooks."""

    PREFIX = "fic_qt_ctx"

    def __init__(self, width, height, B_max, B_min, wK=0, n_iso=1, planes=1, colour=False, device=0):
        self.width, self.height, self.B_max, self.B_min, self.wK, self.n_iso = width, height, B_max, B_min, wK, n_iso
        self.planes, self.colour, self.device = planes, bool(colour), device
        self.cols = 9 if colour else 7
        self.tag = 6 if colour else 2
        h = capi.lib().fic_qt_ctx_create(device, 1 if colour else 0, width, height, B_max, B_min, wK, n_iso, planes)
        (self._encode_threshold, self._encode_budget, self._encode_rd, self._decode, self._collage_host) = self._open(
            h, "encode_threshold", "encode_budget", "encode_rd", "decode_zoom_host", "collage_host")
        self.max_leaves = (width // B_min) * (height // B_min)      # rows per plane of the device leaf table

    # ---- input -----------------------------------------------------------------------------
    def set_gray(self, gray):
        """A grey context's input: uint8 [planes,H,W] numpy array (uploaded once), or a torch CUDA uint8 tensor, used in place
        and read at encode time exactly as Encoder.set_gray's (a misaligned view is cloned here, once)."""
        if hasattr(gray, "data_ptr"):
            return self._set_device(gray, 1, 8, "set_gray_device", "uint8")
        g = np.ascontiguousarray(gray, np.uint8)
        if g.size != self.planes * self.height * self.width:
            raise FicError(-3, f"input has {g.size} pixels, expected {self.planes * self.height * self.width}")
        capi.check(capi.lib().fic_qt_ctx_set_gray_host(self._h, capi.ptr(g, C.c_uint8)))

    def set_argb(self, argb):
        """int32 ARGB [planes,H,W]: a numpy array (either kind of context; a grey one takes the red channel, as Encoder.set_argb),
        or for a colour context a torch CUDA int32 tensor, used in place as RgbEncoder.set_argb's."""
        if hasattr(argb, "data_ptr"):
            return self._set_device(argb, 4, 4, "set_argb_device", "int32")
        a = np.ascontiguousarray(argb, np.int32)
        if a.size != self.planes * self.height * self.width:
            raise FicError(-3, "argb has the wrong number of pixels")
        capi.check(capi.lib().fic_qt_ctx_set_argb_host(self._h, capi.ptr(a, C.c_int32)))

    # ---- compute ---------------------------------------------------------------------------
    def _per_plane(self, v, dtype):
        a = np.asarray(v)
        if a.ndim == 0:
            return np.full(self.planes, v, dtype)
        if a.size != self.planes:
            raise FicError(-3, f"{a.size} values for {self.planes} planes")
        return np.ascontiguousarray(a.reshape(-1), dtype)

    def encode(self, threshold=None, max_leaves=None, max_bytes=None, lam=None, max_sse=None, prune="rd", stream=None):
        """Asynchronous on `stream` (a raw hipStream_t handle / torch stream, None = default).  Exactly one rule, its value a
        scalar for all planes or one per plane: threshold= (the fixed-threshold rule), lam= / max_sse= (rate-distortion pruning,
        DESIGN.md 4.23), max_leaves= / max_bytes= (a stream of the context's format) reached by pruning (prune="rd") or by
        the threshold rule (prune="threshold", DESIGN.md 4.18: the reference criterion only)."""
        if sum(v is not None for v in (threshold, max_leaves, max_bytes, lam, max_sse)) != 1:
            raise ValueError("pass exactly one of threshold=, max_leaves=, max_bytes=, lam= and max_sse=")
        if prune not in ("rd", "threshold"):
            raise ValueError("prune must be 'rd' or 'threshold'")
        s = self._stream(stream)
        if threshold is not None:
            t = self._per_plane(threshold, np.float32)
            capi.check(self._encode_threshold(self._h, capi.ptr(t, C.c_float), s))
            self._threshold_rule = True                       # what results() makes of param: set once the encode is accepted
            return
        if max_bytes is not None:
            b = self._per_plane(max_bytes, np.int64)
            max_leaves = [capi.quadtree_leaves_for_bytes(self.tag, self.n_iso, int(x)) for x in b]
        if max_leaves is not None and prune == "threshold":
            m = self._per_plane(max_leaves, np.int64)
            capi.check(self._encode_budget(self._h, capi.ptr(m, C.c_int64), s))
            self._threshold_rule = True
            return
        goal, v = (capi.QT_RD_LAMBDA, lam) if lam is not None else ((capi.QT_RD_SSE, max_sse) if max_sse is not None else (capi.QT_RD_LEAVES, max_leaves))
        vals = [int(x) for x in (np.asarray(v, object).reshape(-1).tolist() if np.ndim(v) else [v] * self.planes)]
        if len(vals) != self.planes:
            raise FicError(-3, f"{len(vals)} values for {self.planes} planes")
        if any(not 0 <= x < 1 << 64 for x in vals):
            raise FicError(-3, f"{('lam', 'max_leaves', 'max_sse')[goal]}: a value outside 0 .. 2^64 - 1")
        u = np.array(vals, np.uint64)
        capi.check(self._encode_rd(self._h, goal, capi.ptr(u, C.c_uint64), s))
        self._threshold_rule = False

    # ---- results ---------------------------------------------------------------------------
    def results_host(self):
        """(n_leaves int32 [planes], param uint32 [planes], stats uint64 [planes, 4]) of the last encode, one copy
        (fic_qt_ctx_get_results_host).  param: lambda, or the bits of the float32 threshold in force."""
        n, prm, st = np.zeros(self.planes, np.int32), np.zeros(self.planes, np.uint32), np.zeros((self.planes, 4), np.uint64)
        capi.check(capi.lib().fic_qt_ctx_get_results_host(self._h, capi.ptr(n, C.c_int32), capi.ptr(prm, C.c_uint32), capi.ptr(st, C.c_uint64)))
        return n, prm, st

    def results(self, threshold_rule=None):
        """[(leaves int32 [n, cols], param, stats uint64 [4])] per plane, as the one-shot entries return them: param is the
        float32 threshold after an encode under the threshold rule (threshold=, or prune="threshold"), else lambda as an int.
        threshold_rule: None = what the last encode of this object was."""
        n, prm, st = self.results_host()
        if threshold_rule is None:
            threshold_rule = getattr(self, "_threshold_rule", False)
        out = []
        for p in range(self.planes):
            leaves = np.zeros((max(int(n[p]), 1), self.cols), np.int32)
            got = C.c_int()
            capi.check(capi.lib().fic_qt_ctx_get_leaves_host(self._h, p, capi.ptr(leaves, C.c_int32), leaves.shape[0], C.byref(got)))
            out.append((leaves[:got.value].copy(), prm[p:p + 1].view(np.float32)[0] if threshold_rule else int(prm[p]), st[p].copy()))
        return out

    def results_device(self):
        """torch tensors aliasing the context's device results (no copy; the addresses never change): "leaves" int32 [planes,
        max_leaves, cols] (rows of a plane beyond its n_leaves are unspecified), "n_leaves" int32 [planes], "param" int32 [planes]
        (lambda, or the threshold's bits: .view(torch.float32)), "stats" int64 [planes, 4]."""
        import torch
        p = [C.c_void_p() for _ in range(4)]
        capi.check(capi.lib().fic_qt_ctx_result_device_ptrs(self._h, *[C.byref(x) for x in p]))
        dev = torch.device("cuda", self.device)

        def t(ptr, shape, ts):
            return torch.as_tensor(_DevArray(ptr.value, shape, ts), device=dev)

        P = self.planes
        return {"leaves": t(p[0], (P, self.max_leaves, self.cols), "<i4"), "n_leaves": t(p[1], (P,), "<i4"),
                "param": t(p[2], (P,), "<i4"), "stats": t(p[3], (P, 4), "<i8")}

    # ---- decode and collage -------------------------------------------------
    def decode(self, zoom=1):
        """The decoder's loop on every plane of the last encode at once, from the tables on the device
        (fic_qt_ctx_decode_zoom_host).  Returns (images [planes, zoom*H, zoom*W], uint8 for a grey context and packed ARGB int32
        for a colour one, avgError float32 [planes], iterations int32 [planes]); plane p is what the one-shot decoder
        (capi.decode_quadtree_run / decode_rgb_quadtree_iso_run) returns for write_runs()[p] at that zoom."""
        if zoom not in (1, 2, 4):                             # the output is sized from it: refused here, as the library would
            raise FicError(-3, f"zoom={zoom}: only 1, 2 or 4")
        z = int(zoom)
        out = np.zeros((self.planes, z * self.height, z * self.width), np.int32 if self.colour else np.uint8)
        avg, it = np.zeros(self.planes, np.float32), np.zeros(self.planes, np.int32)
        capi.check(self._decode(self._h, z, out.ctypes.data_as(C.c_void_p), out.size, capi.ptr(avg, C.c_float), capi.ptr(it, C.c_int)))
        return out, avg, it

    def collage(self):
        """[planes, H, W] (dtype as decode's): one paint of every plane's leaves from the 2:1 copy of its input image
        (fic_qt_ctx_collage_host) -- the image whose squared distance from the input is stats[p][0]."""
        out = np.zeros((self.planes, self.height, self.width), np.int32 if self.colour else np.uint8)
        capi.check(self._collage_host(self._h, out.ctypes.data_as(C.c_void_p), out.size))
        return out

    def write_runs(self):
        """One stream per plane from the last encode's tables, through the existing writers (tag 2 / tag 6)."""
        runs = []
        for leaves, _, _ in self.results():
            if self.colour:
                runs.append(capi.write_run_rgb_quadtree_iso(leaves, self.width, self.height, self.B_max, self.B_min, self.wK))
            else:
                runs.append(capi.write_run_quadtree(leaves, self.width, self.height, self.B_max, self.B_min, self.wK, self.n_iso))
        return runs


def encode_rgb_per_channel(rgb, B, wK=None, n_iso=1, device=0, sweep=0):
    """BASELINE.json config 5: a batch of colour images encoded as 3 independent grey planes each (NOT the
    reference's joint-RGB fit, which is `capi.encode_rgb`).  rgb: uint8 [N,H,W,3] (or [H,W,3]).
    Returns the result dict with arrays shaped [N, 3, N_r] (qrows [N, 3, N_r, 3]); channel order R, G, B."""
    a = np.ascontiguousarray(rgb, np.uint8)
    if a.ndim == 3:
        a = a[None]
    n, h, w, _ = a.shape
    planes = np.ascontiguousarray(a.transpose(0, 3, 1, 2)).reshape(n * 3, h, w)
    with Encoder(w, h, B, wK, n_iso, n * 3, device) as enc:
        if sweep:
            enc.set_option("sweep", sweep)
        enc.set_gray(planes)
        enc.encode()
        r = enc.results()
    return {k: v.reshape((n, 3) + v.shape[1:]) for k, v in r.items()}


def encode_gray(gray, B, wK=None, n_iso=1, device=0, sweep=0, chunks=0, q_shape=0, search="reference", lsq_engine="valu"):
    """One grey image (uint8 [H,W]) -> result dict with [N_r] arrays (plane axis dropped).  search="lsq": the least-squares
    search (sweep 0 / 1 / 2), with the winners' errors as "E" (int64 [N_r]); lsq_engine="mfma" runs its full
    search on the matrix cores (k_sweep_lsq_q, DESIGN.md 4.21: the same codebook)."""
    g = np.ascontiguousarray(gray, np.uint8)
    with Encoder(g.shape[1], g.shape[0], B, wK, n_iso, 1, device) as enc:
        lsq = capi.search_id(search)
        if lsq:
            enc.set_option("search", lsq)
        if capi.lsq_engine_id(lsq_engine):
            enc.set_option("lsq_engine", lsq_engine)
        if sweep:
            enc.set_option("sweep", sweep)
        if chunks:
            enc.set_option("chunks", chunks)
        if q_shape:
            enc.set_option("q_shape", q_shape)
        enc.set_gray(g)
        enc.encode()
        r = enc.results()
        out = {k: v[0] for k, v in r.items()}
        if lsq:
            out["E"] = enc.lsq_error()[0]
        out["wK"] = enc.wK
        return out


class FractalCompression:
    """Drop-in mirror of bvk_ss19.FractalCompression for the grey encode path.

    Static state like the reference (FC:14-20): set `blockgroesse` / `widthKernel`, call
    `encode(image, out)`.  `n_iso` and `device` are this build's additions (n_iso=1 = reference).
    """

    blockgroesse = 8          # FC:14
    widthKernel = 2           # FC:15
    n_iso = 1                 # extension; 1 == the reference algorithm
    device = 0
    imageInfo = None          # float32 [N_r][3] = {i_local, a, b}   (FC:17,124)
    imageIso = None           # int32 [N_r] winning isometry (extension)
    _last = None

    @staticmethod
    def isGreyScale(image):   # FC:32-45
        rc = capi.lib().fic_is_greyscale_argb(capi.ptr(image.argb, C.c_int32), image.width, image.height)
        return bool(capi.check(rc))

    @classmethod
    def encode(cls, image, out):   # FC:54-59
        if cls.isGreyScale(image):
            return cls.encodeGrayScale(image, out)
        return cls.encodeRGB(image, out)

    avgError = np.float32(0.0)   # FC:20 -- static, never reset between decode calls

    @classmethod
    def getAvgError(cls):   # FC:22-24
        return cls.avgError

    @classmethod
    def decode(cls, inputStream):   # FC:547-553: readInt() isRGB, then the matching decoder on the rest of the stream
        data = inputStream.read() if hasattr(inputStream, "read") else bytes(inputStream)
        if len(data) >= 4 and int.from_bytes(data[:4], "big", signed=True) != 0:      # FC:549-552 -> decodeRGB
            return cls._decode_rgb(data)
        return cls._decode_gray(data)

    @classmethod
    def _decode_gray(cls, run):
        gray, avg, _ = capi.decode_gray_run(run, cls.device, float(cls.avgError))
        cls.avgError = avg
        return RasterImage.from_gray(gray)

    @classmethod
    def _decode_rgb(cls, run):
        argb, avg, _, w, h = capi.decode_rgb_run(run, cls.device, float(cls.avgError))
        cls.avgError = avg
        return RasterImage(w, h, argb)

    @classmethod
    def decodeGreyScale(cls, inputStream):   # FC:356-421: the stream positioned AFTER the isRGB int (as FC.decode leaves it)
        rest = inputStream.read() if hasattr(inputStream, "read") else bytes(inputStream)
        return cls._decode_gray((0).to_bytes(4, "big") + rest)

    @classmethod
    def decodeRGB(cls, inputStream):   # FC:430-508: same convention
        rest = inputStream.read() if hasattr(inputStream, "read") else bytes(inputStream)
        return cls._decode_rgb((1).to_bytes(4, "big") + rest)

    @classmethod
    def generateKernel(cls, domainbloeckePerWidth, domainbloeckePerHeight, index):   # FC:84-100 (host integer logic)
        wK = cls.widthKernel
        dy = index // domainbloeckePerWidth - wK // 2
        dx = index % domainbloeckePerWidth - wK // 2
        dx, dy = max(dx, 0), max(dy, 0)
        if dx + wK >= domainbloeckePerWidth:
            dx = domainbloeckePerWidth - wK
        if dy + wK >= domainbloeckePerHeight:
            dy = domainbloeckePerHeight - wK
        return [dy, dx]

    @staticmethod
    def generateGrayImage(width, height):   # FC:1142-1148
        return RasterImage(width, height, np.full(width * height, np.int32(-8355712)))   # 0xff808080

    _collage = None
    _collageRGB = None

    @classmethod
    def getBestGeneratedCollage(cls, originalImage):   # FC:269-300: the collage of the last encodeGrayScale
        if cls._collage is None or cls._collage.size != originalImage.width * originalImage.height:
            raise FicError(-7, "getBestGeneratedCollage: no grey encode of this image size yet")
        return RasterImage(originalImage.width, originalImage.height, cls._collage.copy())

    @classmethod
    def getBestGeneratedCollageRGB(cls, originalImage):   # FC:308-347
        if cls._collageRGB is None or cls._collageRGB.size != originalImage.width * originalImage.height:
            raise FicError(-7, "getBestGeneratedCollageRGB: no RGB encode of this image size yet")
        return RasterImage(originalImage.width, originalImage.height, cls._collageRGB.copy())

    imageInfoRGB = None       # float32 [N_r][5] = {i_local, a, bR, bG, bB}   (FC:18,185)
    _lastRGB = None

    @classmethod
    def encodeRGB(cls, image, out):   # FC:171-219
        B, wK = cls.blockgroesse, cls.widthKernel
        r = capi.encode_rgb(image.argb, image.width, image.height, B, wK, cls.device, want_collage=True)
        cls.imageInfoRGB = np.stack([r["idx_local"].astype(np.float32), r["a"], r["bR"], r["bG"], r["bB"]], axis=1)
        cls._lastRGB = {"qrows": r["qrows"]}
        cls._collageRGB = np.asarray(r["collage"], np.int32).reshape(-1).copy()
        cls.writeData(out, 1, image.width, image.height)              # FC:217
        return cls.getBestGeneratedCollageRGB(image)                   # FC:218

    @classmethod
    def encodeGrayScale(cls, image, out):   # FC:109-162
        B, wK = cls.blockgroesse, cls.widthKernel
        with Encoder(image.width, image.height, B, wK, cls.n_iso, 1, cls.device) as enc:
            enc.set_argb(image.argb)
            enc.encode()
            r = enc.results()
            cls.imageInfo = np.stack([r["idx_local"][0].astype(np.float32), r["a"][0], r["b"][0]], axis=1)
            cls.imageIso = r["iso"][0].copy()
            cls._last = {"qrows": r["qrows"][0].copy(), "w": image.width, "h": image.height, "B": B, "wK": wK}
            cls._collage = np.asarray(enc.collage()[0], np.int32).reshape(-1).copy()
            cls.writeData(out, 0, image.width, image.height)          # FC:160
        return cls.getBestGeneratedCollage(image)                      # FC:161

    @classmethod
    def writeData(cls, out, isRGB, width, height):   # FC:230-261
        if isRGB != 0:                                               # FC:248-257
            if cls._lastRGB is None:
                raise FicError(-7, "writeData before encode")
            out.write(capi.write_run_rgb(cls._lastRGB["qrows"], width, height, cls.blockgroesse, cls.widthKernel))
            if hasattr(out, "close") and not isinstance(out, io.BytesIO):
                out.close()
            return
        if cls._last is None:
            raise FicError(-7, "writeData before encode")
        run = capi.write_run_gray(cls._last["qrows"], width, height, cls.blockgroesse, cls.widthKernel)
        out.write(run)
        if hasattr(out, "close") and not isinstance(out, io.BytesIO):
            out.close()                                               # FC:259
