"""The device-resident encode path of the handle API: the caller's tensors (fic_ctx_set_gray_device /
fic_rgb_ctx_set_argb_device), the caller's streams, the aliased result and record pointers -- what bench.py times and what
INTEGRATION.md offers to a PyTorch host.  Every codebook is compared bit for bit (idx_local, iso, qrows, the bits of a / b, E under
the least-squares search) with a CPU reference of the image that should have been encoded: the oracle for the reference's search
(rgbisomodel, which is built on it, for colour with 8 isometries), tests/lsqmodel.py and tests/rgblsqmodel.py for "search" =
"lsq".  Only the "device run equals host run" assertions compare two runs of the library.

Shapes: the smallest that reach each loader of the caller's pointer -- 64x64 B = 8 (fused k_prep_q8, 8-byte loads), 32x32 B = 4
and 64x64 B = 16 (k_range_q, 4-byte loads), 64x64 B = 8 through sweeps 2 and 5 (k_range), 48x32 B = 4 with a window
(k_sweep_generic) -- with three different planes, so the plane stride W * H in the caller's buffer matters.

The stream tests rest on one property of PyTorch: a torch.cuda.Stream() is created non-blocking, it does NOT synchronise
implicitly with the null stream (nor with another such stream).  Work queued behind a long filler on such a stream is therefore
still pending when the host goes on, and an encode that ran on the null stream, a getter that did not wait for the caller's
stream, or a second encode that overtook the first one on another stream shows as another image's rows.  The filler is torch
work on that stream; every test that leans on it brackets it with events, brackets an encode on the idle stream the same way
and fails unless the filler lasted at least 100 times the encode."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geomcases as gc  # noqa: E402
import lsqmodel as lm  # noqa: E402
import rgbisomodel as rim  # noqa: E402
import rgblsqmodel as rlm  # noqa: E402

import fic_amd  # noqa: E402
from fic_amd import capi, synth  # noqa: E402
from conftest import GOLDEN, same_f32  # noqa: E402
from oracle import fic_oracle as fo  # noqa: E402

pytestmark = pytest.mark.gpu
E_ARGUMENT = -3

# (w, h, B, wK or None for the full search, search, sweep, n_iso)
GREY = [(64, 64, 8, None, "reference", 6, 1), (64, 64, 8, None, "reference", 6, 8),       # k_prep_q8: uint2 loads
        (32, 32, 4, None, "reference", 6, 1), (32, 32, 4, None, "reference", 6, 8),       # k_range_q: dword loads
        (64, 64, 16, None, "reference", 6, 1), (64, 64, 16, None, "reference", 6, 8),
        (64, 64, 8, None, "reference", 2, 1), (64, 64, 8, None, "reference", 2, 8),       # k_range with copies
        (64, 64, 8, None, "reference", 5, 8),                                             # k_range without, k_range_d4
        (48, 32, 4, 3, "reference", 1, 1), (48, 32, 4, 3, "reference", 1, 8),             # k_sweep_generic
        (64, 64, 8, None, "lsq", 0, 1), (64, 64, 8, None, "lsq", 0, 8), (48, 32, 4, 3, "lsq", 1, 8)]
GREY_IDS = [f"{c[0]}x{c[1]}-B{c[2]}-{c[4]}-sweep{c[5]}-iso{c[6]}" for c in GREY]
KERNEL = {6: "k_sweep_q", 2: "k_sweep_fast", 5: "k_sweep_d4", 1: "k_sweep_generic"}
# colour: 64x64, B = 8, full search (wK = 13), planes = 2: (search, sweep, n_iso)
RGB = [("reference", 1, 1), ("reference", 1, 8), ("reference", 2, 1), ("reference", 2, 8), ("lsq", 0, 1), ("lsq", 0, 8)]
RGB_IDS = [f"{c[0]}-sweep{c[1]}-iso{c[2]}" for c in RGB]
RW, RH, RB, RWK, RP = 64, 64, 8, 13, 2
GREY_STREAM = [GREY[1], GREY[12]]                              # the default sweep and the least-squares search, 8 isometries
RGB_STREAM = [RGB[3], RGB[5]]


# ---- images and references ------------------------------------------------------------------------------------------------------
def grey_planes(w, h, which):
    """uint8 [3, h, w]: three different images; `which` = 0, 1, 2 gives three sets that differ in every plane."""
    lena = np.load(os.path.join(GOLDEN, "lena64.npy"))
    crops = [lena[:h, :w], lena.T[64 - h:, 64 - w:], lena[::-1, ::-1][:h, :w]]
    u, s = synth.image_u(w, h, 101 + which), synth.image_s(w, h, 211 + which)
    order = [(u, s, crops[0]), (s, crops[1], u), (crops[2], u, s)][which]
    return np.ascontiguousarray(np.stack(order), np.uint8)


def rgb_planes(which):
    """int32 [2, h*w] ARGB: two different colour images per set, three sets."""
    kinds = [("U", "lena"), ("S", "U"), ("lena", "S")][which]
    return np.stack([gc.argb_image(k, RW, RH, 11 + 12 * which, p) for p, k in enumerate(kinds)])


_REF = {}


def grey_want(g, B, wK, n_iso, search):
    h, w = g.shape
    key = ("grey", g.tobytes(), w, h, B, wK, n_iso, search)
    if key not in _REF:
        if search == "lsq":
            m = lm.encode(g, B, wK, n_iso)
            _REF[key] = {k: m[k] for k in ("idx_local", "iso", "qrows", "a", "b", "E")}
        else:
            r = fo.encode_gray(fo.gray_to_argb(g), w, h, B, fo.geometry(w, h, B)[2] if wK is None else wK, n_iso)
            _REF[key] = {"idx_local": r["info"][:, 0].astype(np.int32), "iso": r["iso"], "qrows": fo.quantise_gray(r["info"]),
                         "a": r["info"][:, 1], "b": r["info"][:, 2]}
    return _REF[key]


def rgb_want(argb, n_iso, search):
    key = ("rgb", argb.tobytes(), n_iso, search)
    if key not in _REF:
        if search == "lsq":
            m = rlm.encode(argb, RW, RH, RB, RWK, n_iso)
            _REF[key] = {k: m[k] for k in ("idx_local", "iso", "qrows", "a", "bR", "bG", "bB", "E")}
        else:
            if n_iso == 1:
                info = fo.encode_rgb(np.ascontiguousarray(argb), RW, RH, RB, RWK)
                iso, qrows = np.zeros(len(info), np.int32), fo.quantise_rgb(info)
            else:
                r = rim.encode(argb, RW, RH, RB, RWK, 8)
                info, iso, qrows = r["info"], r["iso"], r["qrows"]
            _REF[key] = {"idx_local": info[:, 0].astype(np.int32), "iso": iso, "qrows": qrows, "a": info[:, 1],
                         "bR": info[:, 2], "bG": info[:, 3], "bB": info[:, 4]}
    return _REF[key]


def results(enc, search):
    r = enc.results()
    if search == "lsq":
        r["E"] = enc.lsq_error()
    return r


def assert_rows(got, want, p, what):
    """Plane p of a result dict against a reference dict, bit for bit."""
    for f, v in want.items():
        if v.dtype == np.float32:
            assert same_f32(got[f][p], v), f"{what}: plane {p}: bits of {f}"
        else:
            bad = np.nonzero(np.asarray(got[f][p]).reshape(len(v), -1) != np.asarray(v).reshape(len(v), -1))[0]
            assert bad.size == 0, f"{what}: plane {p}: {f} differs in {bad.size} rows, first at range block {bad[0]}"


def assert_grey(got, imgs, case, what, rows=None):
    w, h, B, wK, search, sweep, n_iso = case
    for p, g in enumerate(imgs):
        want = grey_want(g, B, wK, n_iso, search)
        if rows is not None:
            want = {k: v[rows] for k, v in want.items()}
            assert_rows({k: v[:, rows] for k, v in got.items()}, want, p, what)
        else:
            assert_rows(got, want, p, what)


def assert_rgb(got, argbs, case, what):
    search, sweep, n_iso = case
    for p, argb in enumerate(argbs):
        assert_rows(got, rgb_want(argb, n_iso, search), p, what)


def holds(check, got, imgs, case):
    """True when `got` is the codebook of `imgs` (for a message that says whose rows a failed test found)."""
    try:
        check(got, imgs, case, "")
    except AssertionError:
        return False
    return True


def assert_same_run(a, b, what):
    """Two runs of the library, every field, bit for bit."""
    assert a.keys() == b.keys()
    for k in a:
        if a[k].dtype == np.float32:
            assert same_f32(a[k], b[k]), f"{what}: bits of {k}"
        else:
            assert (a[k] == b[k]).all(), f"{what}: {k}"


def grey_encoder(case, planes=3):
    w, h, B, wK, search, sweep, n_iso = case
    enc = fic_amd.Encoder(w, h, B, wK, n_iso, planes)
    enc.set_option("search", search)
    enc.set_option("sweep", sweep)
    return enc


def rgb_encoder(case):
    search, sweep, n_iso = case
    enc = capi.RgbEncoder(RW, RH, RB, RWK, planes=RP, n_iso=n_iso)
    enc.set_option("search", search)
    enc.set_option("sweep", sweep)
    return enc


def check_kernel(enc, case):
    w, h, B, wK, search, sweep, n_iso = case
    name = enc.last_kernel()
    if search == "lsq":
        assert name == ("k_sweep_lsq_fast" if wK is None else "k_sweep_lsq_generic")
    else:
        assert name.startswith(KERNEL[sweep]), name
        assert ("k_prep_q8" in name) == (sweep == 6 and B == 8), name      # the fused prep: the 8-byte loads of the caller's rows


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- the filler -------------------------------------------------------------------------------------------------------------------
_FILL = {}


class Filler:
    """Elementwise torch work on a stream, bracketed by events: far longer than a 64x64 encode."""
    def __init__(self, stream, ops=1000):
        import torch
        self.torch, self.stream, self.ops = torch, stream, ops
        if "x" not in _FILL:
            _FILL["x"] = torch.zeros(64 << 20, dtype=torch.float32, device="cuda")      # 256 MB: read and written by every op
            _FILL["small"] = torch.zeros(1024, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
        self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def enqueue(self):
        with self.torch.cuda.stream(self.stream):
            self.e0.record()
            for _ in range(self.ops):
                _FILL["x"].add_(1.0)
            self.e1.record()

    def require_margin(self, encode, what):
        """`encode(stream)` once more, on the now idle stream, between events: the filler lasted 100 times as long, or the
        test that relied on it proves nothing and fails."""
        torch = self.torch
        self.stream.synchronize()
        fill_ms = self.e0.elapsed_time(self.e1)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(self.stream)
        encode(self.stream)
        b.record(self.stream)
        b.synchronize()
        enc_ms = a.elapsed_time(b)
        print(f"\nfiller / encode ({what}): {fill_ms:.3f} ms / {enc_ms:.4f} ms = {fill_ms / enc_ms:.0f}")
        assert fill_ms >= 100 * enc_ms, (f"{what}: the filler lasted {fill_ms:.3f} ms, the encode {enc_ms:.4f} ms: less than 100 "
                                         "times as long, so the ordering this test checks was not put under strain")


def stream_beside(other):
    """A new torch stream on which pending work does not hold up work on `other`.  Streams share a few hardware queues, and two
    that share one run in submission order whatever their flags: the races these tests set up could not happen on such a pair,
    and the tests would pass whatever the library did.  So: a short filler on the candidate, one small kernel and an event on
    `other`; the pair serves when that event completes while the filler is still running."""
    import torch
    for attempt in range(16):
        S = torch.cuda.Stream()
        probe = Filler(S, ops=150)
        probe.enqueue()
        done = torch.cuda.Event()
        with torch.cuda.stream(other):
            _FILL["small"].add_(1.0)
            done.record()
        done.synchronize()
        beside = not probe.e1.query()
        S.synchronize()
        if beside:
            print(f"\nstream_beside: candidate {attempt + 1} runs beside the other stream")
            return S
    pytest.fail("16 new torch streams, and work on the other stream waited for the work pending on each of them: "
                "no two streams run side by side here, so no ordering can be put under strain")


# ---- a. device input is what gets encoded -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GREY, ids=GREY_IDS)
def test_grey_device_tensor_is_what_gets_encoded(case):
    w, h = case[:2]
    X, Y, Z = (grey_planes(w, h, i) for i in range(3))
    with grey_encoder(case) as enc, grey_encoder(case) as host:
        enc.set_gray(X)
        enc.encode()
        check_kernel(enc, case)
        assert_grey(results(enc, case[4]), X, case, "host image X")
        t = dev(Y)
        enc.set_gray(t)
        enc.encode()
        got = results(enc, case[4])
        assert_grey(got, Y, case, "device tensor Y after host image X")
        host.set_gray(Y)
        host.encode()
        assert_same_run(got, results(host, case[4]), "device tensor against the host setter")
        enc.set_gray(Z)                                        # back to the context's own copy
        enc.encode()
        assert_grey(results(enc, case[4]), Z, case, "host image Z after device tensor Y")
        assert (t.cpu().numpy() == Y).all(), "the caller's tensor was written to"


@pytest.mark.parametrize("case", RGB, ids=RGB_IDS)
def test_rgb_device_tensor_is_what_gets_encoded(case):
    X, Y, Z = (rgb_planes(i) for i in range(3))
    with rgb_encoder(case) as enc, rgb_encoder(case) as host:
        enc.set_argb(X)
        enc.encode()
        if case[0] == "reference":
            assert enc.last_sweep() == case[1]
        assert_rgb(results(enc, case[0]), X, case, "host image X")
        t = dev(Y)
        enc.set_argb(t)
        enc.encode()
        got = results(enc, case[0])
        assert_rgb(got, Y, case, "device tensor Y after host image X")
        host.set_argb(Y)
        host.encode()
        assert_same_run(got, results(host, case[0]), "device tensor against the host setter")
        enc.set_argb(Z)
        enc.encode()
        assert_rgb(results(enc, case[0]), Z, case, "host image Z after device tensor Y")
        assert (t.cpu().numpy() == Y).all(), "the caller's tensor was written to"


# ---- b. no copy: the tensor is read at encode time -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GREY, ids=GREY_IDS)
def test_grey_tensor_is_read_at_encode_time(case):
    import torch
    w, h = case[:2]
    X, Y = grey_planes(w, h, 0), grey_planes(w, h, 1)
    S = torch.cuda.Stream()
    with grey_encoder(case) as enc:
        t, y = dev(X), dev(Y)
        enc.set_gray(t)
        enc.encode(stream=S)
        assert_grey(results(enc, case[4]), X, case, "tensor holding X")
        with torch.cuda.stream(S):
            t.copy_(y)                                         # in place, on the stream of the encode; no set_gray
        enc.encode(stream=S)
        assert_grey(results(enc, case[4]), Y, case, "the same tensor overwritten with Y")


@pytest.mark.parametrize("case", RGB, ids=RGB_IDS)
def test_rgb_tensor_is_read_at_encode_time(case):
    import torch
    X, Y = rgb_planes(0), rgb_planes(1)
    S = torch.cuda.Stream()
    with rgb_encoder(case) as enc:
        t, y = dev(X), dev(Y)
        enc.set_argb(t)
        enc.encode(stream=S)
        assert_rgb(results(enc, case[0]), X, case, "tensor holding X")
        with torch.cuda.stream(S):
            t.copy_(y)
        enc.encode(stream=S)
        assert_rgb(results(enc, case[0]), Y, case, "the same tensor overwritten with Y")


# ---- c. a caller's stream is honoured --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GREY_STREAM, ids=[GREY_IDS[GREY.index(c)] for c in GREY_STREAM])
def test_grey_encode_runs_on_the_callers_stream(case):
    import torch
    w, h, search = case[0], case[1], case[4]
    X, Y, Z = (grey_planes(w, h, i) for i in range(3))
    S = stream_beside(torch.cuda.default_stream())             # an encode on the null stream would not wait for the filler
    fill = Filler(S)
    with grey_encoder(case) as enc:
        t, y, z = dev(X), dev(Y), dev(Z)
        enc.set_gray(t)
        enc.encode(stream=S)                                   # every lazily allocated store exists from here on
        assert_grey(results(enc, search), X, case, "warm-up")
        enc.set_option("time_sweep", 1)
        fill.enqueue()
        with torch.cuda.stream(S):
            t.copy_(y)
        enc.encode(stream=S)
        got = results(enc, search)                             # no host synchronisation before this getter
        assert_grey(got, Y, case, "encode queued behind the filler and the copy of Y on the caller's stream")
        ms, n = enc.sweep_time()
        assert n == 1 and ms > 0
        # the aliased device arrays, read in stream order without a host synchronisation
        with torch.cuda.stream(S):
            t.copy_(z)
            enc.encode(stream=S)
            rec = enc.records_device().clone()
            d = {k: v.clone() for k, v in enc.results_device().items()}
        S.synchronize()
        got = results(enc, search)
        assert_grey(got, Z, case, "second encode on the caller's stream")
        host = enc.results()
        assert_same_run({k: v.cpu().numpy() for k, v in d.items()}, host, "results_device() clones against results()")
        back = fic_amd.unpack_records(rec.cpu().numpy())
        assert_same_run(back, {k: host[k] for k in back}, "unpack_records(records_device()) against results()")
        fill.require_margin(lambda s: enc.encode(stream=s), f"caller's stream, grey {search}")


@pytest.mark.parametrize("case", RGB_STREAM, ids=[RGB_IDS[RGB.index(c)] for c in RGB_STREAM])
def test_rgb_encode_runs_on_the_callers_stream(case):
    import torch
    X, Y = rgb_planes(0), rgb_planes(1)
    S = stream_beside(torch.cuda.default_stream())
    fill = Filler(S)
    with rgb_encoder(case) as enc:
        t, y = dev(X), dev(Y)
        enc.set_argb(t)
        enc.encode(stream=S)
        assert_rgb(results(enc, case[0]), X, case, "warm-up")
        fill.enqueue()
        with torch.cuda.stream(S):
            t.copy_(y)
        enc.encode(stream=S)
        assert_rgb(results(enc, case[0]), Y, case, "encode queued behind the filler and the copy of Y on the caller's stream")
        fill.require_margin(lambda s: enc.encode(stream=s), f"caller's stream, colour {case[0]}")


# ---- d. two streams, one context ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GREY_STREAM, ids=[GREY_IDS[GREY.index(c)] for c in GREY_STREAM])
def test_grey_second_stream_waits_for_the_first(case):
    """The encode of t1 is queued behind the filler on A, the encode of t2 goes to B at once: the context's stores are shared,
    so B's work must start after A's, and t2's rows are what is left."""
    import torch
    w, h, search = case[0], case[1], case[4]
    X, Y = grey_planes(w, h, 0), grey_planes(w, h, 1)
    B = torch.cuda.Stream()
    A = stream_beside(B)
    fill = Filler(A)
    with grey_encoder(case) as enc:
        t1, t2 = dev(X), dev(Y)
        enc.set_gray(grey_planes(w, h, 2))
        enc.encode()                                           # every lazily allocated store exists from here on
        enc.sync()
        fill.enqueue()
        enc.set_gray(t1)
        enc.encode(stream=A)
        enc.set_gray(t2)
        enc.encode(stream=B)
        got = results(enc, search)
        assert_grey(got, Y, case, "t2 on stream B right after t1 behind the filler on stream A")
        A.synchronize()
        after = results(enc, search)
        assert not holds(assert_grey, after, X, case), "once stream A has drained the context holds t1's rows: A's encode ran after B's"
        assert_same_run(after, got, "after stream A has drained")
        fill.require_margin(lambda s: enc.encode(stream=s), f"two streams, grey {search}")


@pytest.mark.parametrize("case", RGB_STREAM, ids=[RGB_IDS[RGB.index(c)] for c in RGB_STREAM])
def test_rgb_second_stream_waits_for_the_first(case):
    import torch
    X, Y = rgb_planes(0), rgb_planes(1)
    B = torch.cuda.Stream()
    A = stream_beside(B)
    fill = Filler(A)
    with rgb_encoder(case) as enc:
        t1, t2 = dev(X), dev(Y)
        enc.set_argb(rgb_planes(2))
        enc.encode()
        enc.sync()
        fill.enqueue()
        enc.set_argb(t1)
        enc.encode(stream=A)
        enc.set_argb(t2)
        enc.encode(stream=B)
        got = results(enc, case[0])
        assert_rgb(got, Y, case, "t2 on stream B right after t1 behind the filler on stream A")
        A.synchronize()
        after = results(enc, case[0])
        assert not holds(assert_rgb, after, X, case), "once stream A has drained the context holds t1's rows: A's encode ran after B's"
        assert_same_run(after, got, "after stream A has drained")
        fill.require_margin(lambda s: enc.encode(stream=s), f"two streams, colour {case[0]}")


# ---- e. two contexts, two streams, no synchronisation between them ----------------------------------------------------------------------------
def test_two_grey_contexts_on_two_streams_share_nothing():
    import torch
    case = GREY[1]
    X, Y = grey_planes(64, 64, 0), grey_planes(64, 64, 1)
    S1, S2 = torch.cuda.Stream(), torch.cuda.Stream()
    with grey_encoder(case) as e1, grey_encoder(case) as e2:
        e1.set_gray(dev(X))
        e2.set_gray(dev(Y))
        for _ in range(2):                                     # the second round finds every store allocated
            e1.encode(stream=S1)
            e2.encode(stream=S2)
            assert_grey(results(e1, "reference"), X, case, "context 1 on stream 1")
            assert_grey(results(e2, "reference"), Y, case, "context 2 on stream 2")


@pytest.mark.parametrize("rgb_case", RGB_STREAM, ids=[RGB_IDS[RGB.index(c)] for c in RGB_STREAM])
def test_a_grey_and_a_colour_context_on_two_streams_share_nothing(rgb_case):
    import torch
    case = GREY[1]
    X, Y = grey_planes(64, 64, 0), rgb_planes(1)
    S1, S2 = torch.cuda.Stream(), torch.cuda.Stream()
    with grey_encoder(case) as e1, rgb_encoder(rgb_case) as e2:
        e1.set_gray(dev(X))
        e2.set_argb(dev(Y))
        for _ in range(2):
            e1.encode(stream=S1)
            e2.encode(stream=S2)
            assert_grey(results(e1, "reference"), X, case, "grey context on stream 1")
            assert_rgb(results(e2, rgb_case[0]), Y, rgb_case, "colour context on stream 2")


# ---- f. result and record pointers are stable -----------------------------------------------------------------------------------------------------
def result_addresses(enc):
    p = [C.c_void_p() for _ in range(7)]
    capi.check(capi.lib().fic_ctx_result_device_ptrs(enc._h, *[C.byref(x) for x in p]))
    r = C.c_void_p()
    capi.check(capi.lib().fic_ctx_records_device_ptr(enc._h, C.byref(r)))
    return [x.value for x in p] + [r.value]


def test_result_and_record_pointers_never_move():
    """bench.py aliases records_device() once and reads it after every step: the tensors taken before the first encode show the
    rows of every later one, whatever sweep, search, chunk count or lazily allocated store that encode used."""
    case = (64, 64, 8, None, "reference", 0, 8)
    lsq = case[:4] + ("lsq", 0, 8)
    X, Y = grey_planes(64, 64, 0)[:2], grey_planes(64, 64, 1)[:2]
    with fic_amd.Encoder(64, 64, 8, None, 8, planes=2) as enc:
        d0, rec0, addr0 = enc.results_device(), enc.records_device(), result_addresses(enc)
        assert all(addr0) and len(set(addr0)) == 8

        def still_aliased(what):
            host = enc.results()                               # waits for the stream of the last encode
            assert result_addresses(enc) == addr0, f"{what}: a result pointer moved"
            assert_same_run({k: v.cpu().numpy() for k, v in d0.items()}, host, f"{what}: tensors taken before the first encode")
            back = fic_amd.unpack_records(rec0.cpu().numpy())
            assert_same_run(back, {k: host[k] for k in back}, f"{what}: records taken before the first encode")
            return host

        enc.set_gray(X)
        for sweep in (2, 6, 5, 1):
            enc.set_option("sweep", sweep)
            enc.encode()
            assert enc.last_kernel().startswith(KERNEL[sweep])
            assert_grey(still_aliased(f"sweep {sweep}"), X, case, f"sweep {sweep}")
        enc.set_option("sweep_stats", 1)                       # allocates the counters
        enc.set_option("sweep", 6)
        enc.encode()
        assert_grey(still_aliased("sweep_stats on"), X, case, "sweep_stats on")
        enc.sweep_stats()
        enc.set_option("sweep_stats", 0)                       # releases them
        enc.encode()
        assert_grey(still_aliased("sweep_stats off"), X, case, "sweep_stats off")
        enc.set_option("sweep", 0)
        enc.set_option("search", "lsq")
        for chunks in (1, enc.n_domains):                      # the slot stores grow with the chunk count: released and allocated anew
            enc.set_option("chunks", chunks)
            enc.encode()
            assert (enc.info()["chunks"] == 1) == (chunks == 1)    # (chunks are whole pairs of pool blocks: fewer than asked for)
            host = still_aliased(f"lsq, chunks {chunks}")
            host["E"] = enc.lsq_error()
            assert_grey(host, X, lsq, f"lsq, chunks {chunks}")
        enc.set_option("chunks", 0)
        enc.set_option("search", "reference")
        enc.encode()
        assert_grey(still_aliased("back to the reference's search"), X, case, "back to the reference's search")
        b, c = 17, 30                                          # a span inside the 64 range blocks, of another image
        enc.set_gray(Y)
        enc.encode(b, c)
        host = still_aliased("span encode")
        span, rest = np.arange(b, b + c), np.r_[0:b, b + c:64]
        assert_grey(host, Y, case, "span encode, inside the span", rows=span)
        assert_grey(host, X, case, "span encode, outside the span", rows=rest)
        enc.collage()
        still_aliased("collage")
        enc.decode()
        assert_grey(still_aliased("decode"), Y, case, "after collage and decode, inside the span", rows=span)


# ---- g. the alignment contract ------------------------------------------------------------------------------------------------------------------------
def test_grey_misaligned_device_pointer_is_refused():
    """Raw fic_ctx_set_gray_device: an address that is no multiple of 8 is refused before it is stored (no kernel ever sees
    it), the error names the alignment and the input in force stays."""
    import torch
    case = GREY[1]
    X, Y = grey_planes(64, 64, 0), grey_planes(64, 64, 1)
    n = X.size
    L = capi.lib()
    with grey_encoder(case) as enc:
        t = dev(X)
        buf = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
        assert t.data_ptr() % 8 == 0 and buf.data_ptr() % 8 == 0
        enc.set_gray(t)
        for off in (1, 2, 4):
            buf[off:off + n].copy_(dev(Y).reshape(-1))
            torch.cuda.synchronize()
            rc = L.fic_ctx_set_gray_device(enc._h, C.c_void_p(buf.data_ptr() + off))
            assert rc == E_ARGUMENT, f"base + {off} was not refused (rc = {rc}); not encoding with it"
            assert "alignment" in capi.last_error()
            enc.encode()
            assert_grey(results(enc, "reference"), X, case, f"after the refusal of base + {off}: the earlier tensor stays in force")


@pytest.mark.parametrize("w,h,B", [(32, 32, 4), (64, 64, 8), (64, 64, 16)])
def test_grey_device_pointer_at_base_plus_8_is_accepted(w, h, B):
    import torch
    Y = grey_planes(w, h, 1)
    n = Y.size
    buf = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0                            # so base + 8 is a multiple of 8 and of nothing more
    buf[8:8 + n].copy_(dev(Y).reshape(-1))
    torch.cuda.synchronize()
    for sweep in (6, 2):
        case = (w, h, B, None, "reference", sweep, 8)
        with grey_encoder(case) as enc:
            capi.check(capi.lib().fic_ctx_set_gray_device(enc._h, C.c_void_p(buf.data_ptr() + 8)))
            enc.encode()
            check_kernel(enc, case)
            assert_grey(results(enc, "reference"), Y, case, f"base + 8, sweep {sweep}")


@pytest.mark.parametrize("sweep", [6, 2])
def test_grey_view_at_an_odd_offset_is_cloned(sweep):
    """Encoder.set_gray(buf[1:1 + n]): the wrapper hands the library an aligned clone and keeps it alive."""
    import torch
    case = (64, 64, 8, None, "reference", sweep, 8)
    Y = grey_planes(64, 64, 1)
    n = Y.size
    buf = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    view = buf[1:1 + n]
    view.copy_(dev(Y).reshape(-1))
    torch.cuda.synchronize()
    assert view.data_ptr() % 8 == 1
    with grey_encoder(case) as enc:
        enc.set_gray(view)
        assert enc._keep is not view and enc._keep.data_ptr() % 8 == 0, "a misaligned pointer would reach the kernels; not encoding"
        enc.encode()
        assert_grey(results(enc, "reference"), Y, case, "one-byte-offset view")
        aligned = buf[8:8 + n]                                 # an aligned view stays zero-copy
        enc.set_gray(aligned)
        assert enc._keep is aligned


def test_rgb_device_pointer_alignment():
    import torch
    case = RGB[3]
    X, Y = rgb_planes(0), rgb_planes(1)
    n = X.size
    L = capi.lib()
    with rgb_encoder(case) as enc:
        t = dev(X)
        big = torch.zeros(n + 16, dtype=torch.int32, device="cuda")
        assert big.data_ptr() % 8 == 0
        big[1:1 + n].copy_(dev(Y).reshape(-1))
        torch.cuda.synchronize()
        enc.set_argb(t)
        for off in (1, 2, 5):
            rc = L.fic_rgb_ctx_set_argb_device(enc._h, C.c_void_p(big.data_ptr() + off))
            assert rc == E_ARGUMENT, f"base + {off} was not refused (rc = {rc}); not encoding with it"
            assert "alignment" in capi.last_error()
            enc.encode()
            assert_rgb(results(enc, case[0]), X, case, f"after the refusal of base + {off}: the earlier tensor stays in force")
        capi.check(L.fic_rgb_ctx_set_argb_device(enc._h, C.c_void_p(big.data_ptr() + 4)))      # one int32 into a larger tensor
        enc.encode()
        assert_rgb(results(enc, case[0]), Y, case, "base + 4")
        view = big[1:1 + n]
        enc.set_argb(view)                                     # the wrapper: aligned to 4, used in place
        assert enc._keep is view
