"""ctypes binding of libfic_hip.so (include/fic.h).  Fails loudly when the library is missing:
there is no Python or CPU fallback for the hot path."""
import ctypes as C
import os
import sys
import re

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_HERE, "libfic_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "fic.h")

FIC_OK = 0
ERROR_NAMES = {
    -1: "FIC_E_GEOMETRY", -2: "FIC_E_WINDOW", -3: "FIC_E_ARGUMENT", -4: "FIC_E_NO_DEVICE",
    -5: "FIC_E_HIP", -6: "FIC_E_NOT_GREY", -7: "FIC_E_STATE", -8: "FIC_E_CAPACITY",
}


class FicError(Exception):
    """Raised for every negative return code of the C ABI (the reference throws unchecked
    exceptions in the same situations; CTL:184-186 catches them)."""

    def __init__(self, code, message):
        super().__init__(f"{ERROR_NAMES.get(code, code)}: {message}")
        self.code = code


def declared_symbols():
    """Names of every FIC_API function declared in include/fic.h."""
    text = open(HEADER_PATH).read()
    return sorted(set(re.findall(r"FIC_API\s+[\w\s\*]+?\b(fic_\w+)\s*\(", text)))


_C_TYPES = {"char": C.c_char, "int": C.c_int, "float": C.c_float, "double": C.c_double, "int32_t": C.c_int32, "int64_t": C.c_int64,
            "uint8_t": C.c_uint8, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}
_HANDLE_TYPES = ("void", "fic_ctx", "fic_rgb_ctx", "fic_qt_ctx")       # pointers to these are c_void_p


def _ctype(decl, what):
    """The ctypes type of one C type as include/fic.h spells it, the parameter's name (and an array suffix, which makes it a
    pointer) included; None for plain void.  A type this does not know is an error, not a default."""
    words = re.sub(r"\[\d*\]", " * ", decl.replace("*", " * ")).split()
    stars = words.count("*")
    base = [x for x in words if x not in ("*", "const")]
    if not base or len(base) > 2:                       # the type, and perhaps the parameter's name
        raise FicError(-3, f"include/fic.h: cannot read the type of '{decl}' ({what})")
    t = base[0]
    if t in _HANDLE_TYPES:
        if stars == 0 and t == "void" and len(base) == 1:
            return None
        if stars == 1:
            return C.c_void_p
        if stars == 2 and t == "void":
            return C.POINTER(C.c_void_p)
    elif t in _C_TYPES:
        if stars == 0:
            return _C_TYPES[t]
        if stars == 1:
            return C.c_char_p if t == "char" else C.POINTER(_C_TYPES[t])
    raise FicError(-3, f"include/fic.h: no ctypes type for '{decl}' ({what})")


def prototypes():
    """{name: (restype, argtypes)} of every FIC_API declaration of include/fic.h: the header is the one statement of the C ABI,
    lib() types every entry from it."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(HEADER_PATH).read(), flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"FIC_API\s+([^;()]*?)\b(fic_\w+)\s*\(([^)]*)\)\s*;", text, flags=re.S):
        args = [] if params.strip() == "void" else [_ctype(p, name) for p in params.split(",")]
        if None in args:
            raise FicError(-3, f"include/fic.h: a void parameter in {name}")
        out[name] = (_ctype(ret, name), args)
    if sorted(out) != declared_symbols():
        raise FicError(-3, "include/fic.h: a FIC_API declaration this parser cannot read: " + ", ".join(sorted(set(declared_symbols()) ^ set(out))))
    return out


_lib = None


def _torch_first():
    """PyTorch-ROCm wheels bundle their own libamdhip64 / libhsa-runtime64; libfic_hip.so uses /opt/rocm's.  Two HIP
    runtimes share a process as long as torch's initialises first -- the other order leaves torch with "No HIP GPUs are
    available".  So when torch is already imported, bring its runtime up before this library's first HIP call.  (A
    process that imports torch only later should call torch.cuda.init() before its first fic call; bench.py and the
    multi-GPU layer import torch at the top.)"""
    t = sys.modules.get("torch")
    if t is not None:
        try:
            if t.cuda.is_available():
                t.cuda.init()
        except Exception:       # a CPU-only box: the library itself reports FIC_E_NO_DEVICE
            pass


def lib():
    global _lib
    if _lib is not None:
        return _lib
    so = os.environ.get("FIC_HIP_SO") or SO_PATH          # FIC_HIP_SO: another build of the same library (A/B runs of kernel variants)
    if not os.path.exists(so):
        raise FicError(-5, f"{so} is missing: build it with __graft_entry__.build() "
                           "(hipcc --offload-arch=gfx950); there is no fallback path")
    _torch_first()
    L = C.CDLL(so)
    for name, (res, args) in prototypes().items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def has_xcheck():
    """True when the library was built with round 1's exact-covariance matrix-core sweeps ("sweep" = 3 / 4; build.py,
    FIC_BUILD_XCHECK, on by default) -- the test-suite's independent cross-checks of the default sweep.  False when the
    library file does not exist (test modules ask this at import time, and a CPU-only run must still collect them); a
    library that exists but fails to load raises, as every other entry does."""
    so = os.environ.get("FIC_HIP_SO") or SO_PATH
    if not os.path.exists(so):
        return False
    return b"+xcheck" in lib().fic_version()


def last_error():
    return lib().fic_last_error().decode("utf-8", "replace")


def check(rc):
    if rc < 0:
        raise FicError(rc, last_error())
    return rc


def ptr(a, t):
    return None if a is None else a.ctypes.data_as(C.POINTER(t))


def aligned_tensor(t, align):
    """`t` itself where its address is a multiple of `align` bytes (the alignment contract of fic_ctx_set_gray_device /
    fic_rgb_ctx_set_argb_device), else a clone of it in a fresh allocation -- torch's are aligned to 256 bytes and more.  The
    clone is finished when this returns: the encode may run on any stream."""
    if t.data_ptr() % align == 0:
        return t
    import torch
    c = t.clone(memory_format=torch.contiguous_format)
    torch.cuda.current_stream(t.device).synchronize()
    if c.data_ptr() % align != 0:
        raise FicError(-3, f"could not obtain a device allocation aligned to {align} bytes")
    return c


def geometry(w, h, B):
    v = [C.c_int() for _ in range(4)]
    check(lib().fic_geometry(w, h, B, *[C.byref(x) for x in v]))
    return tuple(x.value for x in v)


def _decode_run(plain, zoomed, run, header_bytes, what, dtype, device, avg_error_in, zoom):
    """One stream decoder of the C ABI at `zoom`: (pixels [zoom*h * zoom*w] of dtype, avgError float32, iterations, zoom*w,
    zoom*h).  `zoomed` is the entry that takes the zoom argument, `plain` its twin without one (or None), which serves
    zoom = 1.  The output is sized from the header; the library checks everything else."""
    fn = plain if zoom == 1 and plain is not None else zoomed
    buf = np.frombuffer(bytes(run), np.uint8)
    if buf.size < header_bytes:
        raise FicError(-3, f"{what} shorter than its header")
    z = int(zoom)
    w = int.from_bytes(bytes(run[4:8]), "big", signed=True)
    h = int.from_bytes(bytes(run[8:12]), "big", signed=True)
    cap = max(w, 0) * max(h, 0) * (z * z if z in (1, 2, 4) else 1)
    if cap >= 2 ** 31:                  # the library refuses the size (FIC_E_GEOMETRY) before it looks at the buffer
        cap = 0
    out = np.zeros(max(cap, 1), dtype)
    avg = C.c_float(avg_error_in)
    it, wo, ho = C.c_int(), C.c_int(), C.c_int()
    check(fn(ptr(buf, C.c_uint8), buf.size, *((z,) if fn is zoomed else ()), device, ptr(out, C.c_uint8 if dtype == np.uint8 else C.c_int32),
             cap, C.byref(wo), C.byref(ho), C.byref(avg), C.byref(it)))
    return out[:cap], np.float32(avg.value), it.value, wo.value, ho.value


def decode_gray_run(run, device=0, avg_error_in=0.0, zoom=1):
    """FractalCompression.decode on a grey .run stream (FC:547-553, 356-421), on the GPU (fic_decode_gray_run).
    Returns (gray uint8 [H,W], avgError float32 after the call, iterations).  zoom = 2 / 4: the same loop on the geometry
    (zoom*w, zoom*h, zoom*B, wK), [zoom*H, zoom*W] out (fic_decode_gray_run_zoom)."""
    L = lib()
    out, avg, it, w, h = _decode_run(L.fic_decode_gray_run, L.fic_decode_gray_run_zoom, run, 20, "run stream", np.uint8, device, avg_error_in, zoom)
    return out.reshape(h, w), avg, it


SEARCHES = {"reference": 0, "lsq": 1}


def search_id(search):
    """"reference" (the reference's criterion) / "lsq" (least squares), or the option value 0 / 1 itself."""
    if search in SEARCHES:
        return SEARCHES[search]
    if search in (0, 1):
        return int(search)
    raise FicError(-3, f"search must be 'reference' or 'lsq', not {search!r}")


LSQ_ENGINES = {"valu": 0, "mfma": 1}


def lsq_engine_id(engine):
    """"valu" (k_sweep_lsq_fast) / "mfma" (k_sweep_lsq_q), or the option value itself (the library checks it)."""
    return LSQ_ENGINES[engine] if isinstance(engine, str) and engine in LSQ_ENGINES else engine


def encode_gray_oneshot(gray, B, wK, n_iso=1, device=0, search="reference"):
    """The one-shot C entry point fic_encode_gray_u8 (host buffers in and out; what the JNI shim binds).  search="lsq":
    fic_encode_gray_lsq_u8, with the winners' errors as "E" (int64 [N_r]).  An int32 [H, W] input is taken as ARGB pixels
    (the _argb twins)."""
    g = np.asarray(gray)
    argb = g.dtype != np.uint8
    g = np.ascontiguousarray(g, np.int32 if argb else np.uint8)
    h, w = g.shape
    p = ptr(g, C.c_int32 if argb else C.c_uint8)
    Rw, Rh, Dw, Dh = geometry(w, h, B)
    nr = Rw * Rh
    r = {"idx_local": np.zeros(nr, np.int32), "a": np.zeros(nr, np.float32), "b": np.zeros(nr, np.float32),
         "iso": np.zeros(nr, np.int32), "qrows": np.zeros((nr, 3), np.int32)}
    out = [ptr(r["idx_local"], C.c_int32), ptr(r["a"], C.c_float), ptr(r["b"], C.c_float), ptr(r["iso"], C.c_int32),
           ptr(r["qrows"], C.c_int32)]
    L = lib()
    if search_id(search):
        r["E"] = np.zeros(nr, np.int64)
        fn = L.fic_encode_gray_lsq_argb if argb else L.fic_encode_gray_lsq_u8
        check(fn(p, w, h, B, Dw if wK is None else wK, n_iso, device, *out, ptr(r["E"], C.c_int64)))
    else:
        fn = L.fic_encode_gray_argb if argb else L.fic_encode_gray_u8
        check(fn(p, w, h, B, Dw if wK is None else wK, n_iso, device, *out))
    return r


def encode_gray_multi(gray, B, wK, n_iso=1, n_gpus=1, width=None, height=None):
    """fic_encode_gray_u8_multi / fic_encode_gray_argb_multi: one synchronous call, range blocks sharded over the first
    n_gpus devices, RCCL gather in the library (what the JNI host calls on a multi-GPU node).  `gray`: uint8 [H, W], or --
    with width and height given -- the int32 ARGB pixels of RasterImage.argb."""
    if width is not None:
        g = np.ascontiguousarray(gray, np.int32).reshape(-1)
        w, h = int(width), int(height)
        if g.size != w * h:
            raise FicError(-3, "argb has the wrong number of pixels")
        fn, p = lib().fic_encode_gray_argb_multi, ptr(g, C.c_int32)
    else:
        g = np.ascontiguousarray(gray, np.uint8)
        h, w = g.shape
        fn, p = lib().fic_encode_gray_u8_multi, ptr(g, C.c_uint8)
    Rw, Rh, Dw, Dh = geometry(w, h, B)
    nr = Rw * Rh
    r = {"idx_local": np.zeros(nr, np.int32), "a": np.zeros(nr, np.float32), "b": np.zeros(nr, np.float32),
         "iso": np.zeros(nr, np.int32), "qrows": np.zeros((nr, 3), np.int32)}
    check(fn(p, w, h, B, Dw if wK is None else wK, n_iso, n_gpus, ptr(r["idx_local"], C.c_int32), ptr(r["a"], C.c_float),
             ptr(r["b"], C.c_float), ptr(r["iso"], C.c_int32), ptr(r["qrows"], C.c_int32)))
    return r


def release_cache():
    lib().fic_release_cache()


LIVE_MEMORY_FIELDS = ("device_bytes", "device_allocations", "pinned_bytes", "pinned_allocations")


def live_memory():
    """What the library holds right now, process-wide (fic_debug_live_memory): a dict of LIVE_MEMORY_FIELDS, all 0 once every
    context is closed and release_cache() has run."""
    v = (C.c_int64 * 4)()
    check(lib().fic_debug_live_memory(v))
    return dict(zip(LIVE_MEMORY_FIELDS, [int(x) for x in v]))


def decode_rgb_run(run, device=0, avg_error_in=0.0, zoom=1):
    """decodeRGB (FC:430-508) on the GPU.  Returns (argb int32 [H*W], avgError float32, iterations, w, h); zoom = 2 / 4: at the
    zoomed size (fic_decode_rgb_run_zoom)."""
    L = lib()
    return _decode_run(L.fic_decode_rgb_run, L.fic_decode_rgb_run_zoom, run, 20, "run stream", np.int32, device, avg_error_in, zoom)


def encode_rgb(argb, w, h, B, wK, device=0, want_collage=False, n_iso=1, search="reference", lsq_engine="valu"):
    """encodeRGB (FC:171-219) on the GPU.  argb: int32 [h*w].  Returns a dict of [N_r] arrays
    (idx_local, a, bR, bG, bB, iso, qrows [N_r,5]) and, when asked, the collage (int32 [h*w]).  n_iso = 8: the search also
    tries the 8 isometries of the domain block (fic_encode_rgb_iso_argb; `iso` is all 0 with n_iso = 1, the reference path).
    search="lsq": the least-squares search (fic_encode_rgb_lsq_argb), with the winners' errors as "E" (int64 [N_r]);
    lsq_engine="mfma" runs its full search on the matrix cores (k_sweep_lsq_rgb_q, DESIGN.md 4.22: the same codebook) through a
    context of its own -- the one-shot entry and its cached contexts never carry the option."""
    lsq = search_id(search)
    engine = lsq_engine_id(lsq_engine)
    if engine not in (0, 1):
        raise FicError(-3, f"lsq_engine must be 'valu', 'mfma', 0 or 1, not {lsq_engine!r}")
    if lsq and engine:
        with RgbEncoder(w, h, B, wK, 1, device, n_iso) as enc:
            enc.set_option("search", 1)
            enc.set_option("lsq_engine", 1)
            enc.set_argb(np.ascontiguousarray(argb, np.int32).reshape(1, -1))
            enc.encode(with_collage=want_collage)
            r = {k: v[0] for k, v in enc.results().items()}
            r["E"] = enc.lsq_error()[0]
        return r
    Rw, Rh, Dw, Dh = geometry(w, h, B)
    nr = Rw * Rh
    argb = np.ascontiguousarray(argb, np.int32).reshape(-1)
    if argb.size != w * h:
        raise FicError(-3, "argb has the wrong number of pixels")
    r = {"idx_local": np.zeros(nr, np.int32), "a": np.zeros(nr, np.float32), "bR": np.zeros(nr, np.float32),
         "bG": np.zeros(nr, np.float32), "bB": np.zeros(nr, np.float32), "iso": np.zeros(nr, np.int32),
         "qrows": np.zeros((nr, 5), np.int32)}
    col = np.zeros(w * h, np.int32) if want_collage else None
    args = (ptr(argb, C.c_int32), w, h, B, wK, n_iso, device, ptr(r["idx_local"], C.c_int32), ptr(r["a"], C.c_float),
            ptr(r["bR"], C.c_float), ptr(r["bG"], C.c_float), ptr(r["bB"], C.c_float), ptr(r["iso"], C.c_int32),
            ptr(r["qrows"], C.c_int32), ptr(col, C.c_int32))
    if lsq:
        r["E"] = np.zeros(nr, np.int64)
        check(lib().fic_encode_rgb_lsq_argb(*args, ptr(r["E"], C.c_int64)))
    else:
        check(lib().fic_encode_rgb_iso_argb(*args))
    if want_collage:
        r["collage"] = col
    return r


class Handle:
    """What the three handle classes of the C ABI do alike: Encoder and QuadtreeEncoder (host.py) and RgbEncoder
    derive from it.  A subclass names its entries' prefix (fic_ctx / fic_rgb_ctx / fic_qt_ctx), creates the context and hands it
    to _open; its encode calls the entries bound there.  A method whose entry the handle type does not have (the quadtree
    handle has no sweep_time, sweep_stats, last_kernel, lsq_error) raises AttributeError."""

    PREFIX = None
    _h = None
    SWEEP_STATS_FIELDS = ("tiles", "flagged_tiles", "exact_pairs", "waves", "wave_cycles", "wave_ticks", "waves_sampled")

    def _open(self, handle, *per_encode):
        """Takes over the context `handle` (NULL: raises what the creator recorded) and binds, once, the entries an encode calls:
        `per_encode` names them, `sync` comes with them."""
        L = lib()
        if not handle:
            raise FicError(L.fic_last_error_code() or -3, last_error())
        self._h = handle
        self._keep = None                                  # the device tensor in use as input
        self._sync = self._entry("sync")
        return [self._entry(name) for name in per_encode]

    def _entry(self, name):
        return getattr(lib(), f"{self.PREFIX}_{name}")

    def close(self):
        if self._h:
            self._entry("destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @staticmethod
    def _stream(stream):
        """`stream` (a raw hipStream_t handle / torch stream, None = default) as the entries take it."""
        return C.c_void_p(0 if stream is None else int(getattr(stream, "cuda_stream", stream)))

    def _set_device(self, t, itemsize, align, entry, what):
        """A torch CUDA tensor of planes * H * W elements as the input, in place; one at an address that is no multiple of
        `align` bytes is cloned here, once."""
        n = self.planes * self.height * self.width
        if not t.is_cuda or t.element_size() != itemsize or not t.is_contiguous() or t.numel() != n:
            raise FicError(-3, f"device input must be a contiguous {what} CUDA tensor [planes,H,W]")
        t = aligned_tensor(t, align)
        check(self._entry(entry)(self._h, C.c_void_p(t.data_ptr())))
        self._keep = t

    def set_option(self, name, value):
        """The handle's *_set_option.  "search" also takes "reference" / "lsq", "lsq_engine" also "valu" / "mfma"."""
        if name == "search":
            value = search_id(value)
        if name == "lsq_engine":
            value = lsq_engine_id(value)
            if isinstance(value, str):                       # other numbers: the library refuses them (FIC_E_ARGUMENT)
                raise FicError(-3, f"lsq_engine must be 'valu', 'mfma', 0 or 1, not {value!r}")
        check(self._entry("set_option")(self._h, name.encode(), int(value)))

    def sync(self):
        check(self._sync(self._h))

    def sweep_time(self, reset=True):
        """(total ms, launches) of the sweep launches since the last reset (set_option("time_sweep", 1))."""
        ms, n = C.c_double(), C.c_int()
        check(self._entry("sweep_time")(self._h, C.byref(ms), C.byref(n), 1 if reset else 0))
        return ms.value, n.value

    def sweep_stats(self, reset=True):
        """Counters of the matrix-core sweep (after set_option("sweep_stats", 1)): tile epilogues, flagged tiles, exact pairs,
        waves, and of a sample of the waves the shader-clock cycles / 100 MHz ticks they lived."""
        v = (C.c_uint64 * 8)()
        check(self._entry("sweep_stats")(self._h, v, 1 if reset else 0))
        return dict(zip(self.SWEEP_STATS_FIELDS, [int(x) for x in v]))

    def last_kernel(self):
        """Name of the sweep kernel the last encode launched, as rocprofv3 prints it (without the argument list)."""
        buf = C.create_string_buffer(96)
        check(self._entry("last_kernel")(self._h, buf, 96))
        return buf.value.decode()

    def lsq_error(self):
        """int64 [planes, N_r]: E of the winners of the last encode under set_option("search", "lsq") -- the squared error of
        the quantised map times 10^4 (grey, fic_ctx_get_lsq_error_host) or, over the three channels, times 10^6 (colour,
        fic_rgb_ctx_get_lsq_error_host)."""
        E = np.zeros((self.planes, self.n_ranges), np.int64)
        check(self._entry("get_lsq_error_host")(self._h, ptr(E, C.c_int64)))
        return E

    def _debug_store(self, entry, names, which):
        """Raw bytes (uint8 array) of store `which` of `names` through a *_debug_*_host entry: the size is asked first."""
        fn, i = self._entry(entry), names.index(which)
        size = C.c_int64()
        check(fn(self._h, i, None, 0, C.byref(size)))
        out = np.zeros(size.value, np.uint8)
        check(fn(self._h, i, out.ctypes.data_as(C.c_void_p), out.size, C.byref(size)))
        return out


class RgbEncoder(Handle):
    """Handle API of the joint-RGB path (fic_rgb_ctx_*): `planes` colour images of one geometry, device resident.
    n_iso = 8: the search tries the 8 isometries of every domain block; results()["iso"] holds the winners and decode()
    paints through them.

    Options (set_option): "sweep": 0 auto, 1 the VALU sweeps, 2 the matrix-core full search.  "search": 0 / "reference" or 1 / "lsq" (least
    squares; "sweep" then means 0 auto, 1 generic, 2 fast).  "lsq_tau_widen": 0 (off) or 8..24 --
    diagnostic, > 0 gives WRONG codebooks (the fast least-squares sweep's bound times 1 + 2^-value).  "lsq_engine": 0 / "valu"
    or 1 / "mfma" (the matrix-core sweep k_sweep_lsq_rgb_q, DESIGN.md 4.22: the same codebooks, B = 16 included);
    "lsq_q_eshift": -12..4, diagnostic, > 0 gives WRONG codebooks (that sweep's allowance times 2^-value); "time_sweep": 1
    brackets the least-squares sweep launch with events (sweep_time)."""

    PREFIX = "fic_rgb_ctx"

    def __init__(self, width, height, B, wK, planes=1, device=0, n_iso=1):
        self.width, self.height, self.B, self.wK, self.planes, self.device = width, height, B, wK, planes, device
        self.n_iso = n_iso
        Rw, Rh, Dw, Dh = geometry(width, height, B)
        self.n_ranges = Rw * Rh
        self._encode, = self._open(lib().fic_rgb_ctx_create_iso(device, width, height, B, wK, n_iso, planes), "encode")

    def set_argb(self, argb):
        """int32 [planes, H*W] numpy array (copied) or a torch CUDA int32 tensor of that many elements (used in place and read
        at encode time; one at an address that is no multiple of 4 is cloned here instead, as Encoder.set_gray does)."""
        if hasattr(argb, "data_ptr"):
            return self._set_device(argb, 4, 4, "set_argb_device", "int32")
        a = np.ascontiguousarray(argb, np.int32)
        if a.size != self.planes * self.width * self.height:
            raise FicError(-3, "argb has the wrong number of pixels")
        check(lib().fic_rgb_ctx_set_argb_host(self._h, ptr(a, C.c_int32)))

    def encode(self, with_collage=False, stream=None):
        check(self._encode(self._h, 1 if with_collage else 0, self._stream(stream)))
        self._collage = bool(with_collage)

    def last_sweep(self):
        return check(lib().fic_rgb_ctx_last_sweep(self._h))

    def last_lsq_chunks(self):
        """Pool chunks of the last least-squares sweep (0: the last encode was none)."""
        return check(lib().fic_rgb_ctx_last_lsq_chunks(self._h))

    LSQ_Q_STORES = ("A", "B", "Er", "R")

    def debug_lsq_q(self, which):
        """Raw bytes (uint8 array) of one store of k_lsq_rgb_q_prep after an encode through k_sweep_lsq_rgb_q ("lsq_engine" = 1):
        "A" / "B" the fragments, "Er" the per-range allowance (f32), "R" (u32) (fic_rgb_ctx_debug_lsq_q_host;
        tests/rgblsqqmodel.py decodes them)."""
        return self._debug_store("debug_lsq_q_host", self.LSQ_Q_STORES, which)

    Q_STORES = ("pool", "flat", "rng", "E", "rng_st", "amax")

    def debug_q(self, which):
        """Raw bytes (uint8 array) of one store of the matrix-core RGB sweep for the last plane encoded ("sweep" = 2):
        "pool" / "rng" the A / B fragments, "flat" the flat-tile flags, "E" the per-range error bounds, "rng_st" {0,
        varianzRange} per range, "amax" the largest domain-operand norm (fic_rgb_ctx_debug_q_host; tests/qmodel.py decodes them)."""
        return self._debug_store("debug_q_host", self.Q_STORES, which)

    def results(self):
        P, N = self.planes, self.n_ranges
        r = {"idx_local": np.zeros((P, N), np.int32), "a": np.zeros((P, N), np.float32), "bR": np.zeros((P, N), np.float32),
             "bG": np.zeros((P, N), np.float32), "bB": np.zeros((P, N), np.float32), "qrows": np.zeros((P, N, 5), np.int32)}
        col = np.zeros((P, self.height * self.width), np.int32) if getattr(self, "_collage", False) else None
        check(lib().fic_rgb_ctx_get_results_host(self._h, ptr(r["idx_local"], C.c_int32), ptr(r["a"], C.c_float),
                                                 ptr(r["bR"], C.c_float), ptr(r["bG"], C.c_float), ptr(r["bB"], C.c_float),
                                                 ptr(r["qrows"], C.c_int32), ptr(col, C.c_int32)))
        r["iso"] = np.zeros((P, N), np.int32)
        if self.n_iso != 1:                                  # n_iso = 1: the identity everywhere, the calls of the reference path only
            check(lib().fic_rgb_ctx_get_iso_host(self._h, ptr(r["iso"], C.c_int32)))
        if col is not None:
            r["collage"] = col
        return r

    def decode(self, zoom=1):
        """decodeRGB from the context's quantised rows: (argb int32 [planes, H*W], avgError float32 [planes], iterations).
        zoom = 2 / 4: on the geometry (zoom*w, zoom*h, zoom*B, wK), [planes, zoom*H * zoom*W] out (fic_rgb_ctx_decode_zoom_host)."""
        P, z = self.planes, int(zoom)
        out = np.zeros((P, self.height * self.width * (z * z if z in (1, 2, 4) else 1)), np.int32)
        avg = np.zeros(P, np.float32)
        it = np.zeros(P, np.int32)
        if z == 1:
            check(lib().fic_rgb_ctx_decode_host(self._h, ptr(out, C.c_int32), ptr(avg, C.c_float), ptr(it, C.c_int)))
        else:
            check(lib().fic_rgb_ctx_decode_zoom_host(self._h, z, ptr(out, C.c_int32), ptr(avg, C.c_float), ptr(it, C.c_int)))
        return out, avg, it


def write_run_rgb(qrows5, w, h, B, wK):
    """writeData RGB branch (FC:230-238, 248-257): header + 5 ints per row, big-endian."""
    q = np.ascontiguousarray(qrows5, np.int32).reshape(-1, 5)
    out = np.zeros(20 + 20 * q.shape[0], np.uint8)
    n = lib().fic_write_run_rgb(ptr(q, C.c_int32), q.shape[0], w, h, B, wK, ptr(out, C.c_uint8), out.size)
    check(int(n))
    return out.tobytes()


def write_run_gray(qrows, w, h, B, wK):
    """writeData grey branch (FC:230-246): header + rows, big-endian."""
    q = np.ascontiguousarray(qrows, np.int32).reshape(-1, 3)
    out = np.zeros(20 + 12 * q.shape[0], np.uint8)
    n = lib().fic_write_run_gray(ptr(q, C.c_int32), q.shape[0], w, h, B, wK, ptr(out, C.c_uint8), out.size)
    check(int(n))
    return out.tobytes()


QT_LEAF_FIELDS = ("x", "y", "B", "idx_local", "qa", "qb", "iso")


def _qt_levels(B_max, B_min):
    return [B for B in (16, 8, 4) if B_min <= B <= B_max]


def encode_gray_quadtree(gray, B_max, B_min, wK=0, n_iso=1, threshold=float("inf"), device=0, search="reference"):
    """Quadtree encode of `gray`: uint8 [H, W] (fic_encode_gray_quadtree_u8) or the int32 ARGB pixels of RasterImage.argb as
    [H, W] (fic_encode_gray_quadtree_argb).  wK = 0: full search at every level.  Returns the leaf table int32 [n_leaves, 7] with the columns
    QT_LEAF_FIELDS, in stream order (top-level blocks in scanline order, children TL, TR, BL, BR depth first).
    search="lsq": the per-level codebooks come from the least-squares search (fic_encode_gray_quadtree_lsq_u8 / _argb)."""
    g = np.asarray(gray)
    lsq = search_id(search)
    if g.dtype == np.uint8:
        g = np.ascontiguousarray(g)
        h, w = g.shape
        fn, p = (lib().fic_encode_gray_quadtree_lsq_u8 if lsq else lib().fic_encode_gray_quadtree_u8), ptr(g, C.c_uint8)
    else:
        g = np.ascontiguousarray(g, np.int32)
        h, w = g.shape
        fn, p = (lib().fic_encode_gray_quadtree_lsq_argb if lsq else lib().fic_encode_gray_quadtree_argb), ptr(g, C.c_int32)
    cap = (w // B_min) * (h // B_min) if B_min > 0 and w > 0 and h > 0 else 1
    out = np.zeros((max(cap, 1), 7), np.int32)
    n = C.c_int()
    check(fn(p, w, h, B_max, B_min, wK, n_iso, float(threshold), device, ptr(out, C.c_int32), out.shape[0], C.byref(n)))
    return out[:n.value].copy()


def debug_quadtree_sse(gray, B_max, B_min, wK=0, n_iso=1, device=0):
    """Per-level collage SSE of the quadtree encode: {B: uint32 [Rh, Rw]} for B = B_max .. B_min (fic_debug_quadtree_sse)."""
    g = np.ascontiguousarray(gray, np.uint8)
    h, w = g.shape
    levels = _qt_levels(B_max, B_min)
    sizes = [(h // B) * (w // B) for B in levels]
    out = np.zeros(max(sum(sizes), 1), np.uint32)
    check(lib().fic_debug_quadtree_sse(ptr(g, C.c_uint8), w, h, B_max, B_min, wK, n_iso, device, ptr(out, C.c_uint32), out.size))
    r, o = {}, 0
    for B, n in zip(levels, sizes):
        r[B] = out[o:o + n].reshape(h // B, w // B)
        o += n
    return r


def write_run_quadtree(leaves, w, h, B_max, B_min, wK, n_iso):
    """Quadtree stream (tag 2): header {2, w, h, B_max, B_min, wK, n_iso, n_leaves}, then {B, idx_local, qa, qb[, iso]} per
    leaf, big-endian int32 (fic_write_run_quadtree).  `leaves`: int32 [n, 7] as encode_gray_quadtree returns it."""
    q = np.ascontiguousarray(leaves, np.int32).reshape(-1, 7)
    out = np.zeros(32 + 4 * (5 if n_iso == 8 else 4) * q.shape[0], np.uint8)
    n = lib().fic_write_run_quadtree(ptr(q, C.c_int32), q.shape[0], w, h, B_max, B_min, wK, n_iso, ptr(out, C.c_uint8), out.size)
    check(int(n))
    return out.tobytes()


def decode_quadtree_run(run, device=0, avg_error_in=0.0, zoom=1):
    """Decoder of a quadtree stream on the GPU (fic_decode_quadtree_run).  Returns (gray uint8 [H,W], avgError float32 after the
    call, iterations).  zoom = 2 / 4: every leaf {x, y, B} painted as {zoom*x, zoom*y, zoom*B} (fic_decode_quadtree_run_zoom)."""
    L = lib()
    out, avg, it, w, h = _decode_run(L.fic_decode_quadtree_run, L.fic_decode_quadtree_run_zoom, run, 32, "quadtree stream", np.uint8, device,
                                     avg_error_in, zoom)
    return out.reshape(h, w), avg, it


QT_RGB_LEAF_FIELDS = ("x", "y", "B", "idx_local", "q1", "q2", "q3", "q4")


def _argb_image(argb, w, h):
    a = np.ascontiguousarray(argb, np.int32).reshape(-1)
    if a.size != w * h:
        raise FicError(-3, "argb has the wrong number of pixels")
    return a


def encode_rgb_quadtree(argb, w, h, B_max, B_min, wK=0, threshold=float("inf"), device=0, search="reference"):
    """Joint-RGB quadtree encode of the int32 ARGB pixels `argb` ([h*w] or [h, w]; fic_encode_rgb_quadtree_argb).  wK = 0:
    full search at every level.  Returns the leaf table int32 [n_leaves, 8] with the columns QT_RGB_LEAF_FIELDS (q1..q4: the
    level's encode_rgb qrows row), in stream order.  search="lsq": the per-level codebooks come from the least-squares search
    (fic_encode_rgb_quadtree_lsq_argb)."""
    fn = lib().fic_encode_rgb_quadtree_lsq_argb if search_id(search) else lib().fic_encode_rgb_quadtree_argb
    a = _argb_image(argb, w, h)
    cap = (w // B_min) * (h // B_min) if B_min > 0 and w > 0 and h > 0 else 1
    out = np.zeros((max(cap, 1), 8), np.int32)
    n = C.c_int()
    check(fn(ptr(a, C.c_int32), w, h, B_max, B_min, wK, float(threshold), device, ptr(out, C.c_int32), out.shape[0], C.byref(n)))
    return out[:n.value].copy()


def debug_rgb_quadtree_sse(argb, w, h, B_max, B_min, wK=0, device=0):
    """Per-level collage SSE of the colour quadtree encode: {B: uint32 [Rh, Rw]} for B = B_max .. B_min
    (fic_debug_rgb_quadtree_sse)."""
    a = _argb_image(argb, w, h)
    levels = _qt_levels(B_max, B_min)
    sizes = [(h // B) * (w // B) for B in levels]
    out = np.zeros(max(sum(sizes), 1), np.uint32)
    check(lib().fic_debug_rgb_quadtree_sse(ptr(a, C.c_int32), w, h, B_max, B_min, wK, device, ptr(out, C.c_uint32), out.size))
    r, o = {}, 0
    for B, n in zip(levels, sizes):
        r[B] = out[o:o + n].reshape(h // B, w // B)
        o += n
    return r


def write_run_rgb_quadtree(leaves, w, h, B_max, B_min, wK):
    """Colour quadtree stream (tag 3): header {3, w, h, 0, B_max, B_min, wK, n_leaves}, then {B, idx_local, q1, q2, q3, q4} per
    leaf, big-endian int32 (fic_write_run_rgb_quadtree).  `leaves`: int32 [n, 8] as encode_rgb_quadtree returns it."""
    q = np.ascontiguousarray(leaves, np.int32).reshape(-1, 8)
    out = np.zeros(32 + 24 * q.shape[0], np.uint8)
    n = lib().fic_write_run_rgb_quadtree(ptr(q, C.c_int32), q.shape[0], w, h, B_max, B_min, wK, ptr(out, C.c_uint8), out.size)
    check(int(n))
    return out.tobytes()


def decode_rgb_quadtree_run(run, device=0, avg_error_in=0.0, zoom=1):
    """Decoder of a colour quadtree stream on the GPU (fic_decode_rgb_quadtree_run).  Returns (argb int32 [H, W], avgError
    float32 after the call, iterations).  zoom = 2 / 4: at the zoomed size (fic_decode_rgb_quadtree_run_zoom)."""
    L = lib()
    out, avg, it, w, h = _decode_run(L.fic_decode_rgb_quadtree_run, L.fic_decode_rgb_quadtree_run_zoom, run, 32, "colour quadtree stream",
                                     np.int32, device, avg_error_in, zoom)
    return out.reshape(h, w), avg, it


# ---- streams with an isometry column: tags 4 and 5 (fixed B), tag 6 (colour quadtree) --------------------------
def _write_run_iso(fn, rows, iso, QW, w, h, B, wK):
    q = np.ascontiguousarray(rows, np.int32).reshape(-1, QW)
    k = np.ascontiguousarray(iso, np.int32).reshape(-1)
    if k.size != q.shape[0]:
        raise FicError(-3, "one isometry per row")
    out = np.zeros(24 + 4 * (QW + 1) * q.shape[0], np.uint8)
    n = fn(ptr(q, C.c_int32), ptr(k, C.c_int32), q.shape[0], w, h, B, wK, ptr(out, C.c_uint8), out.size)
    check(int(n))
    return out[:int(n)].tobytes()


def write_run_gray_iso(qrows, iso, w, h, B, wK):
    """Grey fixed-B stream with an isometry column (tag 4): header {4, w, h, 0, B, wK}, then {idx_local, qa, qb, iso} per range
    block, big-endian int32 (fic_write_run_gray_iso).  iso: int [N_r] in 0..7 (zeros for an n_iso = 1 codebook)."""
    return _write_run_iso(lib().fic_write_run_gray_iso, qrows, iso, 3, w, h, B, wK)


def write_run_rgb_iso(qrows5, iso, w, h, B, wK):
    """Colour fixed-B stream with an isometry column (tag 5): header {5, w, h, 0, B, wK}, then {idx_local, q1, q2, q3, q4, iso} per
    range block (fic_write_run_rgb_iso)."""
    return _write_run_iso(lib().fic_write_run_rgb_iso, qrows5, iso, 5, w, h, B, wK)


def decode_gray_iso_run(run, device=0, avg_error_in=0.0, zoom=1):
    """Decoder of a tag-4 stream on the GPU (fic_decode_gray_iso_run): (gray uint8 [zoom*H, zoom*W], avgError float32 after the
    call, iterations)."""
    out, avg, it, w, h = _decode_run(None, lib().fic_decode_gray_iso_run, run, 24, "run stream", np.uint8, device, avg_error_in, zoom)
    return out.reshape(h, w), avg, it


def decode_rgb_iso_run(run, device=0, avg_error_in=0.0, zoom=1):
    """Decoder of a tag-5 stream on the GPU (fic_decode_rgb_iso_run): (argb int32 [zoom*H * zoom*W], avgError float32, iterations,
    zoom*w, zoom*h) like decode_rgb_run."""
    return _decode_run(None, lib().fic_decode_rgb_iso_run, run, 24, "run stream", np.int32, device, avg_error_in, zoom)


QT_RGB_ISO_LEAF_FIELDS = QT_RGB_LEAF_FIELDS + ("iso",)


def encode_rgb_quadtree_iso(argb, w, h, B_max, B_min, wK=0, n_iso=8, threshold=float("inf"), device=0, search="reference"):
    """Joint-RGB quadtree encode with n_iso = 1 or 8 isometries (fic_encode_rgb_quadtree_iso_argb): the leaf table int32
    [n_leaves, 9] with the columns QT_RGB_ISO_LEAF_FIELDS, in stream order.  n_iso = 1: encode_rgb_quadtree's rows and iso = 0.
    search="lsq": the per-level codebooks come from the least-squares search (fic_encode_rgb_quadtree_iso_lsq_argb)."""
    fn = lib().fic_encode_rgb_quadtree_iso_lsq_argb if search_id(search) else lib().fic_encode_rgb_quadtree_iso_argb
    a = _argb_image(argb, w, h)
    cap = (w // B_min) * (h // B_min) if B_min > 0 and w > 0 and h > 0 else 1
    out = np.zeros((max(cap, 1), 9), np.int32)
    n = C.c_int()
    check(fn(ptr(a, C.c_int32), w, h, B_max, B_min, wK, n_iso, float(threshold), device, ptr(out, C.c_int32), out.shape[0], C.byref(n)))
    return out[:n.value].copy()


def debug_rgb_quadtree_iso_sse(argb, w, h, B_max, B_min, wK=0, n_iso=8, device=0):
    """Per-level collage SSE of encode_rgb_quadtree_iso: {B: uint32 [Rh, Rw]} (fic_debug_rgb_quadtree_iso_sse)."""
    a = _argb_image(argb, w, h)
    levels = _qt_levels(B_max, B_min)
    sizes = [(h // B) * (w // B) for B in levels]
    out = np.zeros(max(sum(sizes), 1), np.uint32)
    check(lib().fic_debug_rgb_quadtree_iso_sse(ptr(a, C.c_int32), w, h, B_max, B_min, wK, n_iso, device, ptr(out, C.c_uint32), out.size))
    r, o = {}, 0
    for B, n in zip(levels, sizes):
        r[B] = out[o:o + n].reshape(h // B, w // B)
        o += n
    return r


def write_run_rgb_quadtree_iso(leaves, w, h, B_max, B_min, wK):
    """Colour quadtree stream with an isometry column (tag 6): header {6, w, h, 0, B_max, B_min, wK, n_leaves}, then {B, idx_local,
    q1, q2, q3, q4, iso} per leaf (fic_write_run_rgb_quadtree_iso).  `leaves`: int32 [n, 9] as encode_rgb_quadtree_iso returns it."""
    q = np.ascontiguousarray(leaves, np.int32).reshape(-1, 9)
    out = np.zeros(32 + 28 * q.shape[0], np.uint8)
    n = lib().fic_write_run_rgb_quadtree_iso(ptr(q, C.c_int32), q.shape[0], w, h, B_max, B_min, wK, ptr(out, C.c_uint8), out.size)
    check(int(n))
    return out.tobytes()


def decode_rgb_quadtree_iso_run(run, device=0, avg_error_in=0.0, zoom=1):
    """Decoder of a tag-6 stream on the GPU (fic_decode_rgb_quadtree_iso_run): (argb int32 [zoom*H, zoom*W], avgError float32
    after the call, iterations)."""
    out, avg, it, w, h = _decode_run(None, lib().fic_decode_rgb_quadtree_iso_run, run, 32, "colour quadtree stream", np.int32, device,
                                     avg_error_in, zoom)
    return out.reshape(h, w), avg, it


# ---- quadtree encode to a leaf budget ---------------------------------------------------------------------------
QT_STATS_FIELDS = ("collage_sse", "leaves_B_max", "leaves_B_half", "leaves_B_quarter")


def quadtree_leaves_for_bytes(tag, n_iso, max_bytes):
    """The largest leaf count whose quadtree stream of `tag` (2, 3, 6) fits max_bytes (fic_quadtree_leaves_for_bytes)."""
    return check(int(lib().fic_quadtree_leaves_for_bytes(int(tag), int(n_iso), int(max_bytes))))


def _budget(tag, n_iso, max_leaves, max_bytes):
    if (max_leaves is None) == (max_bytes is None):
        raise ValueError("pass exactly one of max_leaves= and max_bytes=")
    return int(max_leaves) if max_bytes is None else quadtree_leaves_for_bytes(tag, n_iso, max_bytes)


def _encode_budget(fn, head, M, w, h, B_min, cols, device):
    """One budget entry of the C ABI: (leaves int32 [n, cols], threshold float32, stats uint64 [4] as QT_STATS_FIELDS)."""
    cap = (w // B_min) * (h // B_min) if B_min > 0 and w > 0 and h > 0 else 1
    out = np.zeros((max(cap, 1), cols), np.int32)
    n, t, stats = C.c_int(), C.c_float(), np.zeros(4, np.uint64)
    check(fn(*head, M, device, ptr(out, C.c_int32), out.shape[0], C.byref(n), C.byref(t), ptr(stats, C.c_uint64)))
    return out[:n.value].copy(), np.float32(t.value), stats


def encode_gray_quadtree_budget(gray, B_max, B_min, wK=0, n_iso=1, max_leaves=None, max_bytes=None, device=0):
    """encode_gray_quadtree to a size limit: at most max_leaves leaves, or a tag-2 stream of at most max_bytes bytes (exactly
    one of the two), at the smallest threshold that allows it (fic_encode_gray_quadtree_budget_u8 / _argb).  Returns (leaves,
    threshold, stats): the leaf table of encode_gray_quadtree at `threshold` (float32), and uint64 [4] = QT_STATS_FIELDS."""
    M = _budget(2, n_iso, max_leaves, max_bytes)
    g = np.asarray(gray)
    if g.dtype == np.uint8:
        g = np.ascontiguousarray(g)
        fn, p = lib().fic_encode_gray_quadtree_budget_u8, ptr(g, C.c_uint8)
    else:
        g = np.ascontiguousarray(g, np.int32)
        fn, p = lib().fic_encode_gray_quadtree_budget_argb, ptr(g, C.c_int32)
    h, w = g.shape
    return _encode_budget(fn, (p, w, h, B_max, B_min, wK, n_iso), M, w, h, B_min, 7, device)


def encode_rgb_quadtree_budget(argb, w, h, B_max, B_min, wK=0, max_leaves=None, max_bytes=None, device=0):
    """encode_rgb_quadtree to a size limit (tag 3; fic_encode_rgb_quadtree_budget_argb): (leaves [n, 8], threshold, stats)."""
    M = _budget(3, 1, max_leaves, max_bytes)
    a = _argb_image(argb, w, h)
    return _encode_budget(lib().fic_encode_rgb_quadtree_budget_argb, (ptr(a, C.c_int32), w, h, B_max, B_min, wK), M, w, h, B_min, 8, device)


def encode_rgb_quadtree_iso_budget(argb, w, h, B_max, B_min, wK=0, n_iso=8, max_leaves=None, max_bytes=None, device=0):
    """encode_rgb_quadtree_iso to a size limit (tag 6; fic_encode_rgb_quadtree_iso_budget_argb): (leaves [n, 9], threshold, stats)."""
    M = _budget(6, n_iso, max_leaves, max_bytes)
    a = _argb_image(argb, w, h)
    return _encode_budget(lib().fic_encode_rgb_quadtree_iso_budget_argb, (ptr(a, C.c_int32), w, h, B_max, B_min, wK, n_iso), M, w, h, B_min, 9,
                          device)


def debug_qt_select(keys, rank, device=0):
    """The budget's radix select on `keys` (uint32 [n]): (key of rank `rank` in descending order, 0 past the last; the smallest
    float32 >= key / 256; the number of keys above it) (fic_debug_qt_select)."""
    k = np.ascontiguousarray(keys, np.uint32).reshape(-1)
    key, t, above = C.c_uint32(), C.c_float(), C.c_int64()
    check(lib().fic_debug_qt_select(device, ptr(k, C.c_uint32), k.size, int(rank), C.byref(key), C.byref(t), C.byref(above)))
    return key.value, np.float32(t.value), above.value


# ---- quadtree encode by rate-distortion pruning -----------------------------------------------------------------
QT_RD_LAMBDA, QT_RD_LEAVES, QT_RD_SSE = 0, 1, 2


def _rd_goal(tag, n_iso, lam, max_leaves, max_bytes, max_sse):
    """(goal, value) of an RD entry from the one keyword given."""
    if sum(v is not None for v in (lam, max_leaves, max_bytes, max_sse)) != 1:
        raise ValueError("pass exactly one of lam=, max_leaves=, max_bytes= and max_sse=")
    if lam is not None:
        goal, value = QT_RD_LAMBDA, int(lam)
    elif max_sse is not None:
        goal, value = QT_RD_SSE, int(max_sse)
    else:
        goal, value = QT_RD_LEAVES, int(max_leaves) if max_bytes is None else quadtree_leaves_for_bytes(tag, n_iso, max_bytes)
    if not 0 <= value < 1 << 64:
        raise FicError(-3, f"{('lam', 'max_leaves', 'max_sse')[goal]} = {value}: outside 0 .. 2^64 - 1")
    return goal, value


def _encode_rd(fn, head, search, goal, value, w, h, B_min, cols, device):
    """One RD entry of the C ABI: (leaves int32 [n, cols], lambda int, stats uint64 [4] as QT_STATS_FIELDS)."""
    cap = (w // B_min) * (h // B_min) if B_min > 0 and w > 0 and h > 0 else 1
    out = np.zeros((max(cap, 1), cols), np.int32)
    n, lam, stats = C.c_int(), C.c_uint32(), np.zeros(4, np.uint64)
    check(fn(*head, search_id(search), goal, value, device, ptr(out, C.c_int32), out.shape[0], C.byref(n), C.byref(lam), ptr(stats, C.c_uint64)))
    return out[:n.value].copy(), int(lam.value), stats


def encode_gray_quadtree_rd(gray, B_max, B_min, wK=0, n_iso=1, search="reference", lam=None, max_leaves=None, max_bytes=None,
                            max_sse=None, device=0):
    """encode_gray_quadtree with the tree that minimises collage SSE + lam * leaves (fic_encode_gray_quadtree_rd_u8 / _argb).
    Exactly one of: lam= (an integer 0 .. 2^32 - 1), max_leaves= / max_bytes= (a tag-2 stream; the smallest lam whose tree
    fits), max_sse= (the tree of fewest leaves whose collage SSE is <= max_sse; T(0) when none is, see stats[0]).  Returns
    (leaves [n, 7], lam, stats uint64 [4] = QT_STATS_FIELDS); the leaves go to write_run_quadtree unchanged."""
    goal, value = _rd_goal(2, n_iso, lam, max_leaves, max_bytes, max_sse)
    g = np.asarray(gray)
    if g.dtype == np.uint8:
        g = np.ascontiguousarray(g)
        fn, p = lib().fic_encode_gray_quadtree_rd_u8, ptr(g, C.c_uint8)
    else:
        g = np.ascontiguousarray(g, np.int32)
        fn, p = lib().fic_encode_gray_quadtree_rd_argb, ptr(g, C.c_int32)
    h, w = g.shape
    return _encode_rd(fn, (p, w, h, B_max, B_min, wK, n_iso), search, goal, value, w, h, B_min, 7, device)


def encode_rgb_quadtree_rd(argb, w, h, B_max, B_min, wK=0, search="reference", lam=None, max_leaves=None, max_bytes=None, max_sse=None,
                           device=0):
    """encode_rgb_quadtree by rate-distortion pruning (tag 3; fic_encode_rgb_quadtree_rd_argb): (leaves [n, 8], lam, stats)."""
    goal, value = _rd_goal(3, 1, lam, max_leaves, max_bytes, max_sse)
    a = _argb_image(argb, w, h)
    return _encode_rd(lib().fic_encode_rgb_quadtree_rd_argb, (ptr(a, C.c_int32), w, h, B_max, B_min, wK), search, goal, value, w, h, B_min, 8, device)


def encode_rgb_quadtree_iso_rd(argb, w, h, B_max, B_min, wK=0, n_iso=8, search="reference", lam=None, max_leaves=None, max_bytes=None,
                               max_sse=None, device=0):
    """encode_rgb_quadtree_iso by rate-distortion pruning (tag 6; fic_encode_rgb_quadtree_iso_rd_argb): (leaves [n, 9], lam, stats)."""
    goal, value = _rd_goal(6, n_iso, lam, max_leaves, max_bytes, max_sse)
    a = _argb_image(argb, w, h)
    return _encode_rd(lib().fic_encode_rgb_quadtree_iso_rd_argb, (ptr(a, C.c_int32), w, h, B_max, B_min, wK, n_iso), search, goal, value, w, h,
                      B_min, 9, device)


def debug_qt_rd_keys(sse, w, h, B_max, B_min, device=0):
    """The pruning's keys and gains of the per-level SSE arrays `sse` ({B: uint32 [Rh, Rw]} as debug_quadtree_sse returns them):
    (e uint32 [n], G int64 [n]), the blocks of B_max first, then those of B_max / 2 (fic_debug_qt_rd_keys)."""
    levels = _qt_levels(B_max, B_min)
    flat = np.ascontiguousarray(np.concatenate([np.asarray(sse[B]).astype(np.uint32).reshape(-1) for B in levels]))
    if [np.asarray(sse[B]).size for B in levels] != [(h // B) * (w // B) for B in levels]:
        raise FicError(-3, "the SSE arrays do not have the levels' sizes")
    n = sum((h // B) * (w // B) for B in levels[:-1])
    keys, gains = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.int64)
    check(lib().fic_debug_qt_rd_keys(device, ptr(flat, C.c_uint32), w, h, B_max, B_min, ptr(keys, C.c_uint32), ptr(gains, C.c_int64)))
    return keys[:n], gains[:n]


def debug_qt_select_weighted(keys, gains, need, device=0):
    """The weighted select on (keys uint32 [n], gains int64 [n]): (the first boundary among the descending distinct keys and 0
    at which the gain of the keys above it reaches `need`, the number of those keys, their gain) (fic_debug_qt_select_weighted)."""
    k = np.ascontiguousarray(keys, np.uint32).reshape(-1)
    g = np.ascontiguousarray(gains, np.int64).reshape(-1)
    if g.size != k.size:
        raise FicError(-3, "keys and gains differ in length")
    key, above, gain = C.c_uint32(), C.c_int64(), C.c_int64()
    check(lib().fic_debug_qt_select_weighted(device, ptr(k, C.c_uint32), ptr(g, C.c_int64), k.size, int(need), C.byref(key), C.byref(above),
                                             C.byref(gain)))
    return key.value, above.value, gain.value
